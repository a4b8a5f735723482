// k_tuner.hpp -- the tuner block's kernel (dvbt_tuner_*, csrc/dvbt_tuner.inc): raw interleaved I/Q as an SDR delivers it (complex64, int16, int8, uint8) to
// complex64 baseband at another rate, in one pass: convert, mix, resample by L/M.
//
//   v[n] = ((float)raw [- 127.5f]) * scale per component, I and Q exchanged first where swap is set
//   z[n] = v[n] cis(top 32 bits of (n inc mod 2^64))                         (skipped where inc == 0)
//   y[m] = sum_{k = nt-1 .. 0} br[b][k] z[n(m) - k]        n(m) = floor(m M / L), b = m M mod L, br[b][k] = h[b + k L]
//
// n and m count from the stream's beginning, so an output is a function of m and of the nt samples in front of n(m) alone, whatever call, workgroup or lane
// it falls into.  Every product and every sum is one rounded float operation (the library is built with -ffp-contract=off); the sum runs in ascending input
// order and the first product starts it.
//
// A workgroup makes TUN_THREADS consecutive outputs per tile.  The at most ceil(255 M / L) + nt samples a tile needs are converted and mixed exactly once, into
// LDS; the raw bytes are read as 16-byte words wherever a whole aligned word lies inside the call's input (a pointer is aligned to one raw sample only, so the
// words are aligned by address, not by index) and sample by sample at its two ends.  The branch table stands in LDS as [k][b]: the lanes of a wavefront read
// tap k of their own branches from consecutive banks where L is a multiple of 32, and lanes on one branch share the word.  A workgroup loads the table once
// and walks `tiles_per_wg` tiles with it.  A sample in front of the call comes from the handle's history of the last TUN_HIST values of z, as in k_clock.hpp,
// and the workgroup behind the compute workgroups writes the history the next call reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_channel.hpp"

namespace dvbt {

constexpr int TUN_THREADS = 256;
constexpr int TUN_MAX_L = 128, TUN_MAX_M = 1024, TUN_MAX_RATIO = 8;      // after reduction; M / L <= TUN_MAX_RATIO
constexpr int TUN_MAX_NT = 320, TUN_MAX_BRANCH_FLOATS = 8192;            // taps per branch, L * nt
constexpr int TUN_HIST = TUN_MAX_NT;                                     // values of z the handle keeps: nt - 1 <= 319 of them lie in front of a call
constexpr long long TUN_MAX_INDEX = 1ll << 48;                           // first_in, and the inputs of one stream
enum { TUN_CF32 = 0, TUN_CS16 = 1, TUN_CS8 = 2, TUN_CU8 = 3 };

struct TunerArgs {
  int L, M, nt, swap;
  float scale;
  unsigned long long inc;
};

__host__ __device__ constexpr int tun_bytes(int fmt) { return fmt == TUN_CF32 ? 8 : fmt == TUN_CS16 ? 4 : 2; }
// samples a tile of TUN_THREADS outputs reads: n(m0 + 255) - n(m0) <= ceil(255 M / L), and nt - 1 in front of n(m0)
inline int tun_tile(int L, int M, int nt) { return ((TUN_THREADS - 1) * M + L - 1) / L + nt; }
inline int tun_br_floats(int L, int nt) { return (L * nt + 1) & ~1; }                                     // (the tile behind the table stays 8-byte aligned)
inline size_t tun_lds_bytes(int L, int M, int nt) { return sizeof(float) * tun_br_floats(L, nt) + sizeof(float2) * tun_tile(L, M, nt); }

// one component: the raw value as a float -> v
template <int FMT> __device__ __forceinline__ float tun_comp(float r, const TunerArgs &a)
{
  if (FMT == TUN_CU8) r = r - 127.5f;                     // exact
  if (FMT == TUN_CF32 && a.scale == 1.0f) return r;       // the bits as they are
  return r * a.scale;
}

// z of the stream's sample n from its raw components
template <int FMT, bool MIX> __device__ __forceinline__ float2 tun_z(float ri, float rq, unsigned long long n, const TunerArgs &a)
{
  const float vr = tun_comp<FMT>(a.swap ? rq : ri, a), vi = tun_comp<FMT>(a.swap ? ri : rq, a);
  if (!MIX) return make_float2(vr, vi);
  float c, s;
  ch_cossin_turns((uint32_t)((n * a.inc) >> 32), c, s);
  return make_float2(vr * c - vi * s, vr * s + vi * c);
}

// sample j of the call, loaded on its own (the pointer is aligned to one raw sample)
template <int FMT> __device__ __forceinline__ void tun_raw(const void *__restrict__ in, long long j, float &ri, float &rq)
{
  if (FMT == TUN_CF32) { const float2 v = ((const float2 *)in)[j]; ri = v.x; rq = v.y; }
  else if (FMT == TUN_CS16) { const short2 v = ((const short2 *)in)[j]; ri = (float)v.x; rq = (float)v.y; }
  else if (FMT == TUN_CS8) { const char2 v = ((const char2 *)in)[j]; ri = (float)(signed char)v.x; rq = (float)(signed char)v.y; }
  else { const uchar2 v = ((const uchar2 *)in)[j]; ri = (float)v.x; rq = (float)v.y; }
}

// sample i of a 16-byte word of raw samples
template <int FMT> __device__ __forceinline__ void tun_unpack(const uint32_t (&w)[4], int i, float &ri, float &rq)
{
  if (FMT == TUN_CF32) { ri = __uint_as_float(w[2 * i]); rq = __uint_as_float(w[2 * i + 1]); }
  else if (FMT == TUN_CS16) { ri = (float)(short)(w[i] & 0xffffu); rq = (float)(short)(w[i] >> 16); }
  else {
    const uint32_t u = w[i >> 1] >> ((i & 1) * 16);
    if (FMT == TUN_CS8) { ri = (float)(signed char)(u & 0xffu); rq = (float)(signed char)((u >> 8) & 0xffu); }
    else { ri = (float)(u & 0xffu); rq = (float)((u >> 8) & 0xffu); }
  }
}

// tile[p] = z of call sample ja + p for 0 <= p < span, where that sample exists (-TUN_HIST <= ja + p < cnt); in[0] is the stream's sample n0
template <int FMT, bool MIX>
__device__ __forceinline__ void tun_stage(float2 *__restrict__ tile, const void *__restrict__ in, const float2 *__restrict__ hist, long long ja, int span,
                                          long long n0, long long cnt, const TunerArgs &a)
{
  constexpr int BPS = tun_bytes(FMT), SPC = 16 / BPS;
  const int tid = (int)threadIdx.x;
  if (ja < 0) {
    const int nh = -ja < (long long)span ? (int)-ja : span;
    for (int p = tid; p < nh; p += TUN_THREADS) { const long long j = ja + p; tile[p] = j >= -TUN_HIST ? hist[TUN_HIST + j] : make_float2(0.f, 0.f); }
  }
  const long long j_lo = ja > 0 ? ja : 0, j_hi = ja + span < cnt ? ja + span : cnt;
  if (j_lo >= j_hi) return;
  const uintptr_t base = (uintptr_t)in, a0 = base + (uintptr_t)j_lo * BPS, ab = a0 & ~(uintptr_t)15;
  const long long jc0 = j_lo - (long long)((a0 - ab) / BPS);                                    // the first word's first sample (in front of j_lo where ab < a0)
  const int nwords = (int)((base + (uintptr_t)j_hi * BPS - ab + 15) / 16);
  for (int c = tid; c < nwords; c += TUN_THREADS) {
    const long long jc = jc0 + (long long)c * SPC;
    if (jc >= j_lo && jc + SPC <= j_hi) {                                                       // the whole word lies inside the call's input
      const uint4 q = *(const uint4 *)((const char *)in + jc * BPS);                              // 16-byte aligned: base + jc BPS = ab + 16 c
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < SPC; i++) {
        float ri, rq;
        tun_unpack<FMT>(w, i, ri, rq);
        tile[jc + i - ja] = tun_z<FMT, MIX>(ri, rq, (unsigned long long)(n0 + jc + i), a);
      }
    } else {
      for (int i = 0; i < SPC; i++) {
        const long long j = jc + i;
        if (j < j_lo || j >= j_hi) continue;
        float ri, rq;
        tun_raw<FMT>(in, j, ri, rq);
        tile[j - ja] = tun_z<FMT, MIX>(ri, rq, (unsigned long long)(n0 + j), a);
      }
    }
  }
}

// One staged sample as ONE 8-byte LDS read.  Left to itself the compiler pairs the reads of neighbouring taps into 16-byte two-address reads, which move
// half the bytes per LDS cycle; a relaxed atomic load is not paired and costs nothing else (no fence, the same bits).
__device__ __forceinline__ float2 tun_lds_sample(const float2 *p)
{
  const unsigned long long w = __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return make_float2(__uint_as_float((unsigned)w), __uint_as_float((unsigned)(w >> 32)));
}

extern __shared__ float4 tun_lds[];

// The first cblocks workgroups: workgroup w makes the tiles w tiles_per_wg .. of the call's nout outputs, output m0 + t into out[t]; in[0] is the stream's
// sample n0 (absolute), the call has cnt of them; br is the branch table as [k][b].  One workgroup behind them writes the history the next call reads: the
// last TUN_HIST values of z of (this call's history, this call's input).  in, out, hist and hist_next do not overlap.
template <int FMT, bool MIX>
__global__ __launch_bounds__(TUN_THREADS) void tuner_kernel(const void *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist,
                                                            float2 *__restrict__ hist_next, const float *__restrict__ br, long long n0, long long cnt,
                                                            unsigned long long m0, long long nout, unsigned cblocks, int tiles_per_wg, TunerArgs a)
{
  const int tid = (int)threadIdx.x;
  if (blockIdx.x >= cblocks) {
    for (int k = tid; k < TUN_HIST; k += TUN_THREADS) {
      const long long j = cnt - TUN_HIST + k;                         // cnt >= TUN_HIST: all from the input; else the old history moves up by cnt
      float2 z;
      if (j >= 0) { float ri, rq; tun_raw<FMT>(in, j, ri, rq); z = tun_z<FMT, MIX>(ri, rq, (unsigned long long)(n0 + j), a); }
      else z = hist[TUN_HIST + j];
      hist_next[k] = z;
    }
    return;
  }
  float *const s_br = (float *)tun_lds;
  float2 *const tile = (float2 *)(s_br + ((a.L * a.nt + 1) & ~1));
  for (int i = tid; i < a.L * a.nt; i += TUN_THREADS) s_br[i] = br[i];
  const long long ntiles = (nout + TUN_THREADS - 1) / TUN_THREADS;
  const long long tl0 = (long long)blockIdx.x * tiles_per_wg, tl1 = tl0 + tiles_per_wg < ntiles ? tl0 + tiles_per_wg : ntiles;
  for (long long tl = tl0; tl < tl1; tl++) {
    const long long t0 = tl * TUN_THREADS;
    const unsigned long long pr = (m0 + (unsigned long long)t0) * (unsigned long long)a.M;     // < 2^57
    const unsigned long long nb = pr / (unsigned)a.L;                                          // n of the tile's first output
    const unsigned r0 = (unsigned)(pr - nb * (unsigned)a.L);
    const int last = nout - t0 < TUN_THREADS ? (int)(nout - t0) - 1 : TUN_THREADS - 1;
    const int span = (int)((r0 + (unsigned)last * (unsigned)a.M) / (unsigned)a.L) + a.nt;      // tile[p] = z[nb - (nt - 1) + p]
    __syncthreads();                                                                           // the table is there / the tile before this one has been read
    tun_stage<FMT, MIX>(tile, in, hist, (long long)nb - (a.nt - 1) - n0, span, n0, cnt, a);
    __syncthreads();
    if (tid <= last) {
      const unsigned u = r0 + (unsigned)tid * (unsigned)a.M, q = u / (unsigned)a.L, b = u - q * (unsigned)a.L;
      const float2 *const x = tile + q;                                                        // x[i] = z[n(m) - (nt - 1) + i]
      const float *const h = s_br + (a.nt - 1) * a.L + b;                                      // h[-i L] = br[b][nt - 1 - i]
      const float2 x0 = tun_lds_sample(x); const float h0 = h[0];
      float yr = h0 * x0.x, yi = h0 * x0.y;
#pragma unroll 4
      for (int i = 1; i < a.nt; i++) {
        const float2 xi = tun_lds_sample(x + i); const float hi = h[-i * a.L];
        yr += hi * xi.x; yi += hi * xi.y;
      }
      out[t0 + tid] = make_float2(yr, yi);
    }
  }
}

}  // namespace dvbt
