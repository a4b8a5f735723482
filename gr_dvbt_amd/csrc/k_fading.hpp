// k_fading.hpp -- the fading block's kernel (dvbt_fading_*, csrc/dvbt_fading.inc): a tapped delay line whose taps fade as sums of sinusoids.
//
//   y[n] = sum_i g_i(n) x[n - d_i]        g_i(n) = G_i(k) + t (G_i(k + 1) - G_i(k)),  k = n >> 6,  t = (n & 63) / 64
//   G_i(k) = los_i + s_i sum_m cis(top 32 bits of (ph_im + inc_im 64 k mod 2^64))       m ascending, the sum starts from 0
//
// n is the sample's absolute index in the stream.  A knot G_i(k) is a function of k and the table alone, a gain of n and its two knots, and a delayed input is
// read with the same load whether it lies in this call's input or in the handle's history (ch_x), so a stream cut into calls of any size gives the bytes of one
// call.  A workgroup owns the FD_TILE samples of a tile aligned on the ABSOLUTE index; it first fills the tile's n_paths x 17 knots into LDS -- neighbouring
// tiles compute the knot they share twice, to the same bits -- and then every lane works on two pairs of samples.
//
// The knots are filled in passes of FD_PASS knots: all lanes evaluate the pass's FD_PASS x M phasors into a staging array laid out [m][knot], then one lane per
// knot adds its M phasors in ascending m.  Lanes that follow each other touch knots that follow each other in both steps, so neither has a bank conflict.
#pragma once
#include "k_channel.hpp"

namespace dvbt {

constexpr int FD_MAX_PATHS = 24;
constexpr int FD_MAX_SINUSOIDS = 32;
constexpr int FD_KNOT = 64;                               // samples between two knots
constexpr int FD_THREADS = 256;
constexpr int FD_TILE = 1024;                             // samples of a workgroup: two pairs per lane
constexpr int FD_TILE_KNOTS = FD_TILE / FD_KNOT + 1;      // 17: the tile's last sample interpolates towards the next tile's first knot
constexpr int FD_PASS = 64;                               // knots of a pass: one wave adds them
constexpr int FD_HIST_BLOCKS = CH_MAX_DELAY / FD_THREADS;
static_assert(FD_TILE == 4 * FD_THREADS && FD_KNOT == 64 && FD_PASS == 64, "the kernel's shifts");

struct FadePath { float los_re, los_im, s; int delay; };  // s = (float)(sigma / sqrt(M))
struct FadeSin { unsigned long long inc, ph; };           // per sample in units of 2^-64 turns; the phase at n = 0

// path i's four products of a lane: the gains of the samples tt[] behind the knots kn[0] (samples 0, 1) and kn[1] (samples 2, 3), times the delayed inputs x[]
__device__ __forceinline__ void fd_products(float2 pr[4], const float2 x[4], const float2 *knots, int i, const float tt[4], const int kn[2])
{
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float2 G0 = knots[i * FD_TILE_KNOTS + kn[h]], G1 = knots[i * FD_TILE_KNOTS + kn[h] + 1];
    const float dr = G1.x - G0.x, di = G1.y - G0.y;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int u = 2 * h + q;
      const float ar = G0.x + tt[u] * dr, ai = G0.y + tt[u] * di;
      pr[u] = make_float2(ar * x[u].x - ai * x[u].y, ar * x[u].y + ai * x[u].x);
    }
  }
}

// The tile's samples behind its knots: lane t works on the pairs at 2 t and 2 t + 512 of the tile, whose first sample is sample `rel` of the call (negative
// where the call begins inside the tile).  EDGE: the general case -- a sample outside the call stands in as the call's nearest one (its loads stay inside the
// call) and is not stored, and every load chooses between the input and the history (ch_x).  Not EDGE: the whole tile and every delayed sample lie in the
// call's input (rel >= CH_MAX_DELAY, rel + FD_TILE <= cnt), so a pair is one load at a 32-bit offset from the tile.  The arithmetic on the samples is the same
// in both, so a sample's bits do not depend on which of the two its call takes.
template <bool EDGE>
__device__ __forceinline__ void fd_samples(const float2 *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist, const float2 *knots,
                                           const FadePath *__restrict__ paths, int n_paths, long long rel, long long cnt, int t)
{
  long long j[4]; bool v[4]; float tt[4]; int kn[2], off[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    off[h] = h * (FD_TILE / 2) + 2 * t;
    kn[h] = off[h] >> 6;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const long long jj = rel + off[h] + q;
      v[2 * h + q] = !EDGE || (jj >= 0 && jj < cnt);
      j[2 * h + q] = !EDGE ? jj : (jj < 0 ? 0 : (jj < cnt ? jj : cnt - 1));
      tt[2 * h + q] = (float)((off[h] + q) & 63) * 0.015625f;
    }
  }
  if (EDGE && !(v[0] || v[1] || v[2] || v[3])) return;
  const float2 *const tile = in + (EDGE ? 0 : rel);
  float2 y[4];
  for (int i = 0; i < n_paths; i++) {
    const FadePath p = paths[i];
    float2 x[4], pr[4];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      if (EDGE) { x[2 * h] = ch_x(in, hist, j[2 * h] - p.delay); x[2 * h + 1] = ch_x(in, hist, j[2 * h + 1] - p.delay); }
      else { const ChPair q = *reinterpret_cast<const ChPair *>(tile + (off[h] - p.delay)); x[2 * h] = make_float2(q.v.x, q.v.y); x[2 * h + 1] = make_float2(q.v.z, q.v.w); }
    }
    fd_products(pr, x, knots, i, tt, kn);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (i == 0) y[u] = pr[u];                                                        // the first path's product starts the sum
      else { y[u].x += pr[u].x; y[u].y += pr[u].y; }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; h++) {
    if (v[2 * h] && v[2 * h + 1]) { ChPair q; q.v = ch_float4{y[2 * h].x, y[2 * h].y, y[2 * h + 1].x, y[2 * h + 1].y}; *reinterpret_cast<ChPair *>(out + j[2 * h]) = q; }
    else if (v[2 * h]) out[j[2 * h]] = y[2 * h];
    else if (v[2 * h + 1]) out[j[2 * h + 1]] = y[2 * h + 1];
  }
}

// The first cblocks workgroups: workgroup b owns the absolute samples tile0 + b FD_TILE ..; in[0] is the stream's sample n0, the call has cnt samples (a tile
// at either end of the call may be partly filled).  The FD_HIST_BLOCKS workgroups behind them write the history the next call reads, as channel_kernel's do.
// in, out, hist and hist_next do not overlap.  paths[n_paths], tab[n_paths][M].
__global__ __launch_bounds__(FD_THREADS) void fading_kernel(const float2 *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist,
                                                            float2 *__restrict__ hist_next, long long n0, long long cnt, long long tile0, unsigned cblocks,
                                                            const FadePath *__restrict__ paths, const FadeSin *__restrict__ tab, int n_paths, int M)
{
  __shared__ float2 knots[FD_MAX_PATHS * FD_TILE_KNOTS];
  __shared__ float2 stage[FD_MAX_SINUSOIDS * FD_PASS];
  const int t = (int)threadIdx.x;
  if (blockIdx.x >= cblocks) {
    const int k = (int)(blockIdx.x - cblocks) * FD_THREADS + t;                       // k < CH_MAX_DELAY: the grid has exactly FD_HIST_BLOCKS such workgroups
    hist_next[k] = ch_x(in, hist, cnt - CH_MAX_DELAY + k);
    return;
  }
  const long long N = tile0 + (long long)blockIdx.x * FD_TILE;                        // a multiple of FD_TILE
  const unsigned long long k0 = (unsigned long long)N >> 6;
  const int nknots = n_paths * FD_TILE_KNOTS;
  for (int base = 0; base < nknots; base += FD_PASS) {
    for (int idx = t; idx < FD_PASS * M; idx += FD_THREADS) {
      const int m = idx >> 6, kk = base + (idx & 63);
      if (kk < nknots) {
        const int i = kk / FD_TILE_KNOTS, k = kk - i * FD_TILE_KNOTS;
        const FadeSin e = tab[i * M + m];
        float c, s;
        ch_cossin_turns((uint32_t)((e.ph + e.inc * ((k0 + (unsigned long long)k) << 6)) >> 32), c, s);
        stage[idx] = make_float2(c, s);                                                // idx = m FD_PASS + the knot's place in the pass
      }
    }
    __syncthreads();
    if (t < FD_PASS && base + t < nknots) {
      float sr = 0.f, si = 0.f;
      for (int m = 0; m < M; m++) { const float2 v = stage[m * FD_PASS + t]; sr += v.x; si += v.y; }
      const FadePath p = paths[(base + t) / FD_TILE_KNOTS];
      knots[base + t] = make_float2(p.los_re + p.s * sr, p.los_im + p.s * si);
    }
    __syncthreads();
  }

  const long long rel = N - n0;
  if (rel >= CH_MAX_DELAY && rel + FD_TILE <= cnt) fd_samples<false>(in, out, hist, knots, paths, n_paths, rel, cnt, t);
  else fd_samples<true>(in, out, hist, knots, paths, n_paths, rel, cnt, t);
}

}  // namespace dvbt
