// k_channel.hpp -- the channel block's kernels (dvbt_channel_*, csrc/dvbt_channel.inc): static echoes, a carrier offset and seeded white Gaussian noise in
// one pass over the samples, and the mean power of a buffer.
//
//   e[n] = x[n] + sum_i a_i x[n - d_i]        r[n] = e[n] exp(2 pi j phi(n))        y[n] = r[n] + sigma (g_re(n) + j g_im(n))
//
// n is the sample's absolute index in the stream.  Nothing a sample goes through depends on the call it arrives in: the noise is a function of (seed, n) -- a
// counter-based generator, Philox4x32-10, whose counter is n >> 1 -- the phase is the 64-bit integer product inc n, and a delayed input is read with the same
// load and enters the same sum whether it lies in this call's input or in the handle's history of the last CH_MAX_DELAY samples.  So a stream cut into calls of
// any size gives the bytes of one call.  One lane works on the two samples 2 P, 2 P + 1 that share Philox block P (pairing by the absolute index's parity: a
// call that begins or ends on an odd n has a half-filled pair at that end), which is also one 128-bit load and one 128-bit store.
//
// The Gaussian pair of a sample comes from two of the block's four words by Box-Muller: u1 = ((w_a >> 9) + 0.5) 2^-23 in (0, 1), u2 = (w_b >> 8) 2^-24 in
// [0, 1), rho = sqrt(-2 ln u1), g = rho (cos, sin)(2 pi u2).  The smallest u1 is 2^-24, so the tails end at rho = sqrt(48 ln 2) = 5.77 sigma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dvbt {

constexpr int CH_MAX_PATHS = 8;
constexpr int CH_MAX_DELAY = 8192;          // samples of history the handle keeps (one 8k symbol)
constexpr int CH_THREADS = 256;
constexpr int CH_HIST_BLOCKS = CH_MAX_DELAY / CH_THREADS;
constexpr int CH_POW_BLOCKS = 1024;         // fixed, so that the order of the power's additions does not depend on the length

struct ChannelArgs {
  int n_paths; int delay[CH_MAX_PATHS]; float are[CH_MAX_PATHS], aim[CH_MAX_PATHS];
  int has_cfo; unsigned long long inc;      // phase increment per sample in units of 2^-64 turns
  float sigma; uint32_t key0, key1;         // sigma == 0: no noise
};

typedef float ch_float4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(8))) ChPair { ch_float4 v; };   // two samples; a pair is 8-byte aligned, 16-byte aligned only where pointer and parity agree

// Philox4x32-10 (Salmon et al., SC'11), the standard multipliers and Weyl constants
__device__ __forceinline__ void ch_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4])
{
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// cos, sin of 2 pi p / 2^32: the nearest quarter turn is taken off as an integer, the rest (|x| <= pi / 4) goes through Taylor polynomials whose first
// omitted terms are 1e-10 and 2e-9.  The low bits of p that a float cannot hold (6 of the remainder's 30) are rounded away: 2e-8 rad.
__device__ __forceinline__ void ch_cossin_turns(uint32_t p, float &c, float &s)
{
  const uint32_t q = (p + 0x20000000u) >> 30;
  const int r = (int)(p - (q << 30));
  const float x = (float)r * 1.4629180792671596e-9f;      // 2 pi / 2^32
  const float z = x * x;
  float sp = __builtin_fmaf(z, 2.7557319e-6f, -1.9841270e-4f);
  sp = __builtin_fmaf(z, sp, 8.3333333e-3f); sp = __builtin_fmaf(z, sp, -1.6666667e-1f);
  const float sn = __builtin_fmaf(x * z, sp, x);
  float cp = __builtin_fmaf(z, -2.7557319e-7f, 2.4801587e-5f);
  cp = __builtin_fmaf(z, cp, -1.3888889e-3f); cp = __builtin_fmaf(z, cp, 4.1666667e-2f); cp = __builtin_fmaf(z, cp, -0.5f);
  const float cs = __builtin_fmaf(z, cp, 1.0f);
  c = (q & 1) ? sn : cs; s = (q & 1) ? cs : sn;
  if ((q + 1) & 2) c = -c;
  if (q & 2) s = -s;
}

// -2 ln u for u in (0, 1): u = 2^e m with m in [sqrt(1/2), sqrt(2)), ln m = 2 atanh((m - 1) / (m + 1)).  m - 1 is exact and e = 0 for u >= sqrt(1/2), so the
// result keeps its relative precision where u approaches 1 (the hardware's log2 is not relied on there)
__device__ __forceinline__ float ch_neg2ln(float u)
{
  const int bits = __float_as_int(u);
  const int e = (bits - 0x3f3504f3) >> 23;
  const float m = __int_as_float(bits - (e << 23));
  const float t = (m - 1.0f) * __builtin_amdgcn_rcpf(m + 1.0f);
  const float z = t * t;
  float p = __builtin_fmaf(z, 0.11111111f, 0.14285714f);
  p = __builtin_fmaf(z, p, 0.2f); p = __builtin_fmaf(z, p, 0.33333333f);
  const float lnm = __builtin_fmaf(t * z, p, t);         // atanh(t)
  const float fe = (float)e;
  // ln u = e ln2_hi (exact: ln2_hi has 16 significant bits) + (e ln2_lo + 2 atanh t)
  const float ln = fe * 0.693145751953125f + __builtin_fmaf(fe, 1.42860677e-6f, 2.0f * lnm);
  return -2.0f * ln;
}

__device__ __forceinline__ float2 ch_gauss(uint32_t wa, uint32_t wb)
{
  const float u1 = ((float)(wa >> 9) + 0.5f) * 1.1920928955078125e-7f;   // exact: an odd multiple of 2^-24
  const float rho = __builtin_amdgcn_sqrtf(ch_neg2ln(u1));
  float c, s;
  ch_cossin_turns(wb & 0xffffff00u, c, s);
  return make_float2(rho * c, rho * s);
}

// sample j of the call (j >= -CH_MAX_DELAY): the call's input, or the history in front of it
__device__ __forceinline__ float2 ch_x(const float2 *__restrict__ in, const float2 *__restrict__ hist, long long j)
{
  return j >= 0 ? in[j] : hist[CH_MAX_DELAY + j];
}

// What the samples of a pair go through behind their own loads, side by side so that the loads and the two chains of arithmetic overlap: e[k] = x[n + k] on
// entry, j[k] = its index in the call, ph = phi(n), w the pair's Philox block.  Each sample's arithmetic is its own: the same whatever its neighbour is.
__device__ __forceinline__ void ch_pair(float2 e[2], const float2 *__restrict__ in, const float2 *__restrict__ hist, const long long j[2], unsigned long long ph,
                                        const uint32_t w[4], const ChannelArgs &a)
{
  for (int i = 0; i < a.n_paths; i++) {
    const float2 d0 = ch_x(in, hist, j[0] - a.delay[i]), d1 = ch_x(in, hist, j[1] - a.delay[i]);
    const float ar = a.are[i], ai = a.aim[i];
    e[0].x += ar * d0.x - ai * d0.y; e[0].y += ar * d0.y + ai * d0.x;
    e[1].x += ar * d1.x - ai * d1.y; e[1].y += ar * d1.y + ai * d1.x;
  }
  if (a.has_cfo) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      float c, s;
      ch_cossin_turns((uint32_t)((ph + (k ? a.inc : 0ull)) >> 32), c, s);
      e[k] = make_float2(e[k].x * c - e[k].y * s, e[k].x * s + e[k].y * c);
    }
  }
  if (a.sigma != 0.f) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const float2 g = ch_gauss(w[2 * k], w[2 * k + 1]);
      e[k].x += a.sigma * g.x; e[k].y += a.sigma * g.y;
    }
  }
}

// The first cblocks workgroups: lane t works on the absolute pair pair0 + t of the call's npairs pairs; in[0] is the stream's sample n0, the call has cnt
// samples.  The CH_HIST_BLOCKS workgroups behind them write the history the next call reads: the last CH_MAX_DELAY samples of (this call's history, this call's
// input).  in, out, hist and hist_next do not overlap.
__global__ __launch_bounds__(CH_THREADS) void channel_kernel(const float2 *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist,
                                                             float2 *__restrict__ hist_next, long long n0, long long cnt, long long pair0, long long npairs,
                                                             unsigned cblocks, ChannelArgs a)
{
  if (blockIdx.x >= cblocks) {
    const int k = (int)(blockIdx.x - cblocks) * CH_THREADS + (int)threadIdx.x;       // k < CH_MAX_DELAY: the grid has exactly CH_HIST_BLOCKS such workgroups
    hist_next[k] = ch_x(in, hist, cnt - CH_MAX_DELAY + k);                          // cnt >= CH_MAX_DELAY: all from the input; else the old history moves up by cnt
    return;
  }
  const long long t = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  if (t >= npairs) return;
  const long long P = pair0 + t;
  const long long j = 2 * P - n0;                      // -1 where the call begins on an odd n
  const bool v0 = j >= 0, v1 = j + 1 < cnt;
  // a half-filled pair at either end of the call: the missing sample stands in as a copy of the present one (its loads stay inside the call) and is not stored
  const long long jj[2] = {v0 ? j : j + 1, v1 ? j + 1 : j};
  float2 e[2];
  if (v0 && v1) { const ChPair q = *reinterpret_cast<const ChPair *>(in + j); e[0] = make_float2(q.v.x, q.v.y); e[1] = make_float2(q.v.z, q.v.w); }
  else { e[0] = in[jj[0]]; e[1] = e[0]; }
  uint32_t w[4] = {0, 0, 0, 0};
  if (a.sigma != 0.f) ch_philox((uint32_t)P, (uint32_t)((unsigned long long)P >> 32), 0u, 0u, a.key0, a.key1, w);
  ch_pair(e, in, hist, jj, a.inc * (unsigned long long)(2 * P), w, a);
  if (v0 && v1) { ChPair q; q.v = ch_float4{e[0].x, e[0].y, e[1].x, e[1].y}; *reinterpret_cast<ChPair *>(out + j) = q; }
  else if (v0) out[j] = e[0];
  else out[j + 1] = e[1];
}

// mean power, first step: workgroup b adds |x[i]|^2 in double over i = b CH_THREADS + lane + k CH_POW_BLOCKS CH_THREADS (k ascending), then its lanes pairwise in
// a fixed tree.  No atomics: the same data give the same bits.
__device__ __forceinline__ double ch_block_sum(double acc, double *sh)
{
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int w = CH_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(CH_THREADS) void channel_power_kernel(const float2 *__restrict__ x, long long n, double *__restrict__ partial)
{
  __shared__ double sh[CH_THREADS];
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x; i < n; i += (long long)CH_POW_BLOCKS * CH_THREADS) {
    const float2 v = x[i];
    acc += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
  }
  const double s = ch_block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// second step, one workgroup: the CH_POW_BLOCKS partial sums in the same fixed order; result[0] = the mean
__global__ __launch_bounds__(CH_THREADS) void channel_power_final_kernel(const double *__restrict__ partial, long long n, double *__restrict__ result)
{
  __shared__ double sh[CH_THREADS];
  double acc = 0.0;
  for (int i = (int)threadIdx.x; i < CH_POW_BLOCKS; i += CH_THREADS) acc += partial[i];
  const double s = ch_block_sum(acc, sh);
  if (threadIdx.x == 0) result[0] = s / (double)n;
}

}  // namespace dvbt
