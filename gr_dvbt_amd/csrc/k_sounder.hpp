// k_sounder.hpp -- the channel sounder's kernels (dvbt_sounder.inc): the echo profile and the amplitude response of the channel from the scattered pilots of
// fft-shifted symbol rows.  The specification stands in include/dvbt_hip.h.
//
// Three kernels per call:
//   sounder_extract_kernel   one workgroup per symbol: the continual-pilot sum c_i (and c_0 of its group, formed again from the group's first row where that
//                            row is in this call, read from the carry where it is not), then the Kp / 4 scattered pilots of the row, timing- and
//                            phase-corrected, into the group's Kp entries E.  A group that the call leaves open goes into the carry instead: its entries, c_0
//                            and four ints (index, offset and cp_start of its first symbol, and whether a symbol so far has broken it).
//   sounder_profile_kernel   one workgroup per RUN of SND_RUN consecutive groups, [SND_RUN r, SND_RUN r + SND_RUN) in the stream's numbering: per used group
//                            the windowed entries into the padded LDS image (components swapped: the forward transform of the swapped input is the swapped
//                            inverse transform, and |.|^2 does not see the swap), fft_dif_lds at M points, |h|^2 and |E|^2 into float accumulators in
//                            registers (thread t owns bins t, t + 512, ...).  A closed run is stored as one slab; a run that the call leaves open is stored as
//                            it stands and the next call's first workgroup starts from it.
//   sounder_fold_kernel      adds the call's slabs in ascending run order into doubles, and their counts of used groups into an integer.
// Every floating-point sum is thereby formed in an order fixed by the stream, never by the call, and there is no atomic in floating point.
#pragma once
#include <stdint.h>
#include "k_fft.hpp"

namespace dvbt {

constexpr int SND_RUN = 8;                         // groups per slab
constexpr int SND_EXTRACT_THREADS = 256;
constexpr int SND_MAX_DELTA = 64;                  // |cp_start - cp_start of the group's first symbol| of a used group

struct SndArgs {
  int N, K, Kp, M, zl, n_cp, first_index;
  int n;                                           // symbols of this call
  long long pos0;                                  // stream position of the call's first symbol
  const float2 *rows;                              // [n][N]
  const int *idx, *off, *cps;                      // [n] each, or null
  const float2 *carry_in;                          // the open group in front of pos0: E[Kp], c_0, then four ints
};

struct SndGroup { int idx0, off0, cps0, bad; };

__host__ __device__ inline size_t snd_carry_float2(int Kp) { return (size_t)Kp + 1 + 2; }        // entries, c_0, four ints
__host__ __device__ inline size_t snd_slab_words(int M, int Kp) { return (size_t)M + Kp + 1; }   // |h|^2 sums, |E|^2 sums, the count of used groups

// index, offset and cp_start of the call's symbol at stream position s >= pos0
__device__ __forceinline__ void snd_meta(const SndArgs &a, long long s, int &x, int &o, int &c)
{
  const long long i = s - a.pos0;
  x = a.idx ? a.idx[i] : (int)((a.first_index + s) % 68);
  o = a.off ? a.off[i] : 0;
  c = a.cps ? a.cps[i] : 0;
}

// group g as far as the symbols in front of s_end tell: its first symbol's values and whether one of them has broken it
__device__ inline SndGroup snd_group(const SndArgs &a, long long g, long long s_end)
{
  SndGroup G;
  const long long s0 = 4 * g;
  int i;
  if (s0 < a.pos0) {
    const int *m = reinterpret_cast<const int *>(a.carry_in + a.Kp + 1);
    G.idx0 = m[0]; G.off0 = m[1]; G.cps0 = m[2]; G.bad = m[3];
    i = (int)(a.pos0 - s0);
  } else {
    snd_meta(a, s0, G.idx0, G.off0, G.cps0);
    G.bad = (G.idx0 < 0 || G.idx0 > 67 || G.off0 < -8 || G.off0 > 7) ? 1 : 0;
    i = 1;
  }
  for (; i < 4 && s0 + i < s_end; i++) {
    int x, o, c;
    snd_meta(a, s0 + i, x, o, c);
    const long long d = (long long)c - (long long)G.cps0;
    if (x != (G.idx0 + i) % 68 || o != G.off0 || d > SND_MAX_DELTA || d < -SND_MAX_DELTA) G.bad = 1;
  }
  return G;
}

// the workgroup's sum of one complex value per thread, in a tree that depends on nothing but the thread numbering (xor-butterflies inside a wave, the
// waves in ascending order); every thread returns it
__device__ __forceinline__ float2 snd_block_sum(float2 v, float2 *s_w, int tid)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { v.x += __shfl_xor(v.x, m, 64); v.y += __shfl_xor(v.y, m, 64); }
  __syncthreads();                                 // s_w may still be read from the call before
  if ((tid & 63) == 0) s_w[tid >> 6] = v;
  __syncthreads();
  float2 s = s_w[0];
#pragma unroll
  for (int w = 1; w < SND_EXTRACT_THREADS / 64; w++) { s.x += s_w[w].x; s.y += s_w[w].y; }
  return s;
}

// tau(k) = cis(-2 pi ((k - c0) delta mod N) / N) out of the FFT's table tw[t] = cis(-2 pi t / N)
__device__ __forceinline__ float2 snd_tau(const float2 *__restrict__ twN, int k, int c0, long long delta, int N)
{
  return twN[(int)(((long long)(k - c0) * delta) & (long long)(N - 1))];
}

// Blocks 0 .. nsym - 1: the symbols at stream positions s_first ..; block nsym (there iff copy_old): the entries that the carry holds of the group that was
// open in front of the call, to where the call's symbols of that group go.
//   ebuf      [groups of this launch][Kp]: group g at (g - g_base) Kp
//   g_open    the group whose entries go to carry_out instead (the one the call leaves open), or -1
__global__ __launch_bounds__(SND_EXTRACT_THREADS) void sounder_extract_kernel(SndArgs a, long long s_first, int nsym, long long g_base, float2 *__restrict__ ebuf,
                                                                              float2 *__restrict__ carry_out, long long g_open, int copy_old,
                                                                              const int16_t *__restrict__ cpilot, const float *__restrict__ pref,
                                                                              const float2 *__restrict__ twN)
{
  __shared__ float2 s_w[SND_EXTRACT_THREADS / 64];
  const int tid = threadIdx.x, Kp = a.Kp;
  const long long s_end = a.pos0 + a.n;
  if ((int)blockIdx.x >= nsym) {                   // the carried entries of the group in front of the call
    if (!copy_old) return;
    const long long g = a.pos0 / 4;
    const int have = (int)(a.pos0 - 4 * g);        // 1 .. 3 symbols
    float2 *dst = g == g_open ? carry_out : ebuf + (size_t)(g - g_base) * Kp;
    const int *m = reinterpret_cast<const int *>(a.carry_in + Kp + 1);
    const int l0 = m[0] & 3;
    for (int j = tid; j < Kp; j += SND_EXTRACT_THREADS)
      if (((j - l0) & 3) < have) dst[j] = a.carry_in[j];
    if (g == g_open && tid == 0) {
      const SndGroup G = snd_group(a, g, s_end);
      int *mo = reinterpret_cast<int *>(carry_out + Kp + 1);
      carry_out[Kp] = a.carry_in[Kp];
      mo[0] = G.idx0; mo[1] = G.off0; mo[2] = G.cps0; mo[3] = G.bad;
    }
    return;
  }
  const long long s = s_first + blockIdx.x, g = s / 4;
  const int i = (int)(s - 4 * g), N = a.N, c0k = (a.K - 1) / 2;
  const SndGroup G = snd_group(a, g, s + 1);       // the group's first symbol (what later symbols say decides nothing here)
  int x, o, c;
  snd_meta(a, s, x, o, c);
  if (o < -8 || o > 7) o = 0;                      // such a group is skipped; its reads stay inside the row
  const int o0 = G.off0 < -8 || G.off0 > 7 ? 0 : G.off0;
  const long long delta = (long long)c - (long long)G.cps0;
  const float2 *row = a.rows + (size_t)(s - a.pos0) * N + a.zl + o;

  // c_i, and c_0 of the group
  float2 ci = make_float2(0.f, 0.f), cz = ci;
  if (tid < a.n_cp) {                              // n_cp <= 177: one continual pilot per thread
    const int k = cpilot[tid];
    const float w = pref[k];
    const float2 y = row[k];
    ci = cmul(make_float2(y.x * w, y.y * w), snd_tau(twN, k, c0k, delta, N));
    if (i > 0 && 4 * g >= a.pos0) {
      const float2 y0 = a.rows[(size_t)(4 * g - a.pos0) * N + a.zl + o0 + k];
      cz = cmul(make_float2(y0.x * w, y0.y * w), twN[0]);   // delta = 0: the very operations of the first symbol's own c_i
    }
  }
  ci = snd_block_sum(ci, s_w, tid);
  if (i == 0) {
    cz = ci;
  } else if (4 * g >= a.pos0) {
    cz = snd_block_sum(cz, s_w, tid);
  } else {
    cz = a.carry_in[Kp];
  }
  // r_i = c_0 conj(c_i) / |c_0 conj(c_i)|, 1 where that is 0 or not finite
  float2 r = make_float2(cz.x * ci.x + cz.y * ci.y, cz.y * ci.x - cz.x * ci.y);
  {
    const float mag = sqrtf(r.x * r.x + r.y * r.y);
    if (mag > 0.f && mag <= 3.4028234e38f) { r.x /= mag; r.y /= mag; } else r = make_float2(1.f, 0.f);
  }

  float2 *dst = g == g_open ? carry_out : ebuf + (size_t)(g - g_base) * Kp;
  const int l = x & 3;
  for (int p = tid; 3 * l + 12 * p < a.K; p += SND_EXTRACT_THREADS) {
    const int k = 3 * l + 12 * p;
    const float w = pref[k] * 0.5625f;             // w_k 9/16: +-3/4
    const float2 y = row[k];
    dst[l + 4 * p] = cmul(cmul(make_float2(y.x * w, y.y * w), snd_tau(twN, k, c0k, delta, N)), r);
  }
  if (i == 0 && g == g_open && tid == 0) {         // the open group starts in this call: its state for the next one
    const SndGroup Ge = snd_group(a, g, s_end);
    int *mo = reinterpret_cast<int *>(carry_out + Kp + 1);
    carry_out[Kp] = cz;
    mo[0] = Ge.idx0; mo[1] = Ge.off0; mo[2] = Ge.cps0; mo[3] = Ge.bad;
  }
}

// One workgroup per run of the launch: run r_first + blockIdx.x, of which the call closes the groups [ka, kb) (clipped to the run).
//   ebuf      group g at (g - g_base) Kp
//   open_in   the open run's state from the previous call (read where ka is inside a run): M + Kp floats and the count
//   open_out  where a run that this call leaves open is stored (another buffer than open_in)
//   slabs     [gridDim.x][M + Kp + 1]: the closed runs of this launch
// NB = M / FFT_THREADS bins and NR = ceil(Kp / FFT_THREADS) carriers per thread.  Only the accumulators live across the transform (see spectrum_kernel).
// Dynamic LDS: the FFT's workspace at M points (fft_lds_bytes(M)).
template <int NB, int NR>
__global__ __launch_bounds__(FFT_THREADS, 4) void sounder_profile_kernel(SndArgs a, const float2 *__restrict__ ebuf, long long g_base, long long r_first,
                                                                         long long ga, long long gb, const float *__restrict__ win,
                                                                         const float2 *__restrict__ twM, const float *__restrict__ open_in,
                                                                         float *__restrict__ open_out, float *__restrict__ slabs)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int M = a.M, Kp = a.Kp, tid = threadIdx.x;
  const FftWork fw = fft_work(smem_raw, M);
  float2 *const x = fw.x;
  fft_work_fill(fw, M, twM, tid);

  const long long r = r_first + blockIdx.x;
  const long long ka = ga > r * SND_RUN ? ga : r * SND_RUN, kb = gb < (r + 1) * SND_RUN ? gb : (r + 1) * SND_RUN;
  const bool from_open = (ka % SND_RUN) != 0, to_open = (kb % SND_RUN) != 0;
  float acc[NB], rsp[NR];
  int used = 0;
#pragma unroll
  for (int j = 0; j < NB; j++) acc[j] = 0.f;
#pragma unroll
  for (int j = 0; j < NR; j++) rsp[j] = 0.f;
  if (from_open) {
#pragma unroll
    for (int j = 0; j < NB; j++) acc[j] = open_in[tid + j * FFT_THREADS];
#pragma unroll
    for (int j = 0; j < NR; j++) { const int b = tid + j * FFT_THREADS; if (b < Kp) rsp[j] = open_in[M + b]; }
    used = reinterpret_cast<const int *>(open_in)[M + Kp];
  }
  __syncthreads();

  for (long long g = ka; g < kb; g++) {
    if (snd_group(a, g, 4 * g + 4).bad) continue;  // the same for every thread
    used++;
    const float2 *E = ebuf + (size_t)(g - g_base) * Kp;
    int t = tid;
    asm volatile("" : "+v"(t));
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int b = t + j * FFT_THREADS;
      float2 v = make_float2(0.f, 0.f);
      if (b < Kp) {
        const float2 e = E[b];
        const float w = win[b];
        v = make_float2(e.y * w, e.x * w);         // swapped
        if (j < NR) rsp[j] = rsp[j] + (e.x * e.x + e.y * e.y);
      }
      x[fpad(b)] = v;
    }
    __syncthreads();
    fft_dif_lds(fw, M, tid);                       // ends behind a barrier
    int u = tid, Mk = M;
    asm volatile("" : "+v"(u), "+s"(Mk));
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const float2 X = x[fpad(fft_pos_of_bin(u + j * FFT_THREADS, Mk))];
      acc[j] = acc[j] + (X.x * X.x + X.y * X.y);
    }
    __syncthreads();
  }

  float *dst = to_open ? open_out : slabs + (size_t)blockIdx.x * snd_slab_words(M, Kp);
#pragma unroll
  for (int j = 0; j < NB; j++) dst[tid + j * FFT_THREADS] = acc[j];
#pragma unroll
  for (int j = 0; j < NR; j++) { const int b = tid + j * FFT_THREADS; if (b < Kp) dst[M + b] = rsp[j]; }
  if (tid == 0) reinterpret_cast<int *>(dst)[M + Kp] = used;
}

// acc[b] += slab_0[b] + slab_1[b] + ... in ascending order, one thread per word of a slab; the last word is the count of used groups (an integer sum)
__global__ __launch_bounds__(256) void sounder_fold_kernel(const float *__restrict__ slabs, int words, int nslabs, double *__restrict__ acc,
                                                           long long *__restrict__ used)
{
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < words - 1) {
    double s = acc[b];
    for (int q = 0; q < nslabs; q++) s += (double)slabs[(size_t)q * words + b];
    acc[b] = s;
  } else if (b == words - 1) {
    long long s = *used;
    for (int q = 0; q < nslabs; q++) s += (long long)reinterpret_cast<const int *>(slabs)[(size_t)q * words + b];
    *used = s;
  }
}

}  // namespace dvbt
