// k_quality.hpp -- blind signal-quality measurement over what a finished segment left in device memory (gfx950, wave64):
// the modulation error ratio of the equalised carriers against the demapper's own decisions, the channel bit errors (the
// decoder's output re-encoded against the decoder's input) and the bit errors the RS decoder removed.  None of these kernels
// is part of the receive chain's launch sequence; they only read its buffers.
//
// Sums: the two MER kernels add floats in a fixed order (per thread in carrier order, a butterfly over the wavefront, the
// four wavefronts in order, then doubles over the symbols in a fixed tree) -- no float atomics, the same bits on every run.
// The bit counters are integers: partial counts per wavefront, one 64-bit atomic add per wavefront and counter, any order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_backend.hpp"

namespace dvbt {

constexpr int Q_THREADS = 256;          // workgroup of every kernel here
constexpr unsigned Q_MAX_GRID = 2048;   // the counting kernels stride their work over at most this many workgroups (8192 atomics per counter at the most)

__device__ __forceinline__ float q_wave_sum(float v)
{
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);      // the same butterfly in every lane: one order of additions
  return v;
}
__device__ __forceinline__ unsigned q_wave_sum(unsigned v)
{
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// One workgroup per output symbol: (sum |ideal|^2, sum |eq - ideal|^2) over the symbol's payload carriers, ideal = the
// constellation point of the label the demapper chose.  eq / labels point at the first output symbol.
__global__ __launch_bounds__(Q_THREADS) void quality_mer_kernel(const float2 *__restrict__ eq, const uint8_t *__restrict__ labels, const float2 *__restrict__ points,
                                                                int payload, float2 *__restrict__ per_symbol)
{
  __shared__ float2 s_pts[64];
  __shared__ float2 s_part[Q_THREADS / 64];
  const int tid = threadIdx.x;
  if (tid < 64) s_pts[tid] = points[tid];
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * payload;
  float sig = 0.f, err = 0.f;
  for (int i = tid; i < payload; i += Q_THREADS) {
    const float2 e = eq[base + i];
    const float2 p = s_pts[labels[base + i] & 63];
    const float dx = e.x - p.x, dy = e.y - p.y;
    sig += p.x * p.x + p.y * p.y;
    err += dx * dx + dy * dy;
  }
  sig = q_wave_sum(sig); err = q_wave_sum(err);
  if ((tid & 63) == 0) s_part[tid >> 6] = make_float2(sig, err);
  __syncthreads();
  if (tid == 0) {
    float2 r = s_part[0];
#pragma unroll
    for (int w = 1; w < Q_THREADS / 64; w++) { r.x += s_part[w].x; r.y += s_part[w].y; }
    per_symbol[blockIdx.x] = r;
  }
}

// One workgroup: the per-symbol pairs added in double, every thread its symbols in index order, then a fixed tree
__global__ __launch_bounds__(Q_THREADS) void quality_sum_kernel(const float2 *__restrict__ per_symbol, int n, double *__restrict__ out /* [2]: signal, error */)
{
  __shared__ double s_sig[Q_THREADS], s_err[Q_THREADS];
  const int tid = threadIdx.x;
  double sig = 0.0, err = 0.0;
  for (int i = tid; i < n; i += Q_THREADS) { const float2 v = per_symbol[i]; sig += (double)v.x; err += (double)v.y; }
  s_sig[tid] = sig; s_err[tid] = err;
  __syncthreads();
  for (int o = Q_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) { s_sig[tid] += s_sig[tid + o]; s_err[tid] += s_err[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { out[0] = s_sig[0]; out[1] = s_err[0]; }
}

// Channel bit errors.  Output byte j of the decoder carries trellis steps 8j .. 8j + 7 (MSB first) of the input stream from its first
// byte.  A thread takes 8 decoded bytes = 64 steps at a time: the encoder's X (171 octal: delays 0,1,2,3,6) and Y (133 octal: delays
// 0,2,3,5,6) outputs of all 64 steps from the 70-bit window of information bits by shifts and XORs, the received bits of the same steps
// gathered from the input bytes (m bits per byte, MSB first) along the puncture pattern, then two XORs and popcounts.  Counted: the
// steps 8 <= t < 8 n_vit (the encoder needs six earlier bits) whose kept bit lies inside the input, q < n_in m.
// counts[0] += counted bits, counts[1] += differing bits.  The result does not depend on the grid: groups are strided over it.
__global__ __launch_bounds__(Q_THREADS) void quality_channel_kernel(const uint8_t *__restrict__ in, long long n_in, const uint8_t *__restrict__ vit, long long n_vit,
                                                                    VitParams vp, unsigned long long *__restrict__ counts)
{
  const long long groups = (n_vit + 7) / 8;
  const unsigned long long q_end = (unsigned long long)n_in * (unsigned)vp.m;
  const unsigned long long t_end = (unsigned long long)n_vit * 8;
  unsigned nbits = 0, nerr = 0;
  for (long long g = (long long)blockIdx.x * Q_THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * Q_THREADS) {
    // W bit j = information bit of step 64 g + j; P = the six bits in front of it at the top of a word (bit 63 = step - 1)
    unsigned long long W = 0;
    if (8 * g + 8 <= n_vit && ((uintptr_t)(vit + 8 * g) & 7) == 0) {
      const unsigned long long le = *reinterpret_cast<const unsigned long long *>(vit + 8 * g);
      W = __builtin_bitreverse64(__builtin_bswap64(le));
    } else {
      for (int b = 0; b < 8; b++) if (8 * g + b < n_vit) W |= (unsigned long long)__builtin_bitreverse8(vit[8 * g + b]) << (8 * b);
    }
    const unsigned long long P = g > 0 ? (unsigned long long)__builtin_bitreverse8(vit[8 * g - 1]) << 56 : 0ull;
#define Q_DELAY(d) ((W << (d)) | (P >> (64 - (d))))
    const unsigned long long s2 = Q_DELAY(2), s3 = Q_DELAY(3), s6 = Q_DELAY(6), common = W ^ s2 ^ s3 ^ s6;
    const unsigned long long X = common ^ Q_DELAY(1), Y = common ^ Q_DELAY(5);
#undef Q_DELAY
    // steps of this group that are counted at all
    const unsigned long long t0 = (unsigned long long)g * 64;
    unsigned long long V = ~0ull;
    if (g == 0) V &= ~0xffull;
    if (t0 + 64 > t_end) V &= (t_end > t0) ? ((1ull << (t_end - t0)) - 1ull) : 0ull;     // (t_end - t0 is a multiple of 8 below 64 here)
    // the received bits: coded position c = 2 t (X), 2 t + 1 (Y); kept where the puncture vector says so; kept bit q = (c / plen) n + prefix[c % plen]
    const unsigned long long c0 = 2 * t0, per = __umul64hi(c0, vp.magic_plen);
    int ph = (int)(c0 - per * (unsigned)vp.plen);
    unsigned long long q = per * (unsigned)vp.n + vp.prefix[ph];
    long long bi = (long long)__umul64hi(q, vp.magic_m);
    int bj = (int)(q - (unsigned long long)bi * (unsigned)vp.m);
    unsigned cur = bi < n_in ? in[bi] : 0u;
    unsigned long long RX = 0, RY = 0, MX = 0, MY = 0;
    for (int j = 0; j < 64; j++) {
#pragma unroll
      for (int xy = 0; xy < 2; xy++) {
        if ((vp.punct_mask >> (ph + xy)) & 1u) {
          if (q < q_end) {
            const unsigned long long bit = (cur >> (vp.m - 1 - bj)) & 1u;
            if (xy == 0) { RX |= bit << j; MX |= 1ull << j; } else { RY |= bit << j; MY |= 1ull << j; }
          }
          q++;
          if (++bj == vp.m) { bj = 0; bi++; cur = bi < n_in ? in[bi] : 0u; }
        }
      }
      ph += 2; if (ph >= vp.plen) ph = 0;
    }
    MX &= V; MY &= V;
    nbits += (unsigned)__builtin_popcountll(MX) + (unsigned)__builtin_popcountll(MY);
    nerr += (unsigned)__builtin_popcountll((X ^ RX) & MX) + (unsigned)__builtin_popcountll((Y ^ RY) & MY);
  }
  nbits = q_wave_sum(nbits); nerr = q_wave_sum(nerr);
  if ((threadIdx.x & 63) == 0) {
    if (nbits) atomicAdd(&counts[0], (unsigned long long)nbits);
    if (nerr) atomicAdd(&counts[1], (unsigned long long)nerr);
  }
}

// Post-Viterbi bit errors: what the RS decoder changed in the 188 data bytes of every word.  The word as received is regathered from the
// Viterbi stream (the byte de-interleaver in closed form: byte p of the de-interleaved stream is byte p - 204 (11 - p % 12) of the Viterbi
// stream, zero in front of it), so the DEINT tap need not exist.  A thread handles 4 data bytes of one word (47 threads per word).
// counts[0] += differing bits.  Words the decoder gave up on pass through unchanged and add nothing.
__global__ __launch_bounds__(Q_THREADS) void quality_rs_kernel(const uint8_t *__restrict__ vit, long long n_vit, const uint8_t *__restrict__ rs_out, long long n_words,
                                                               unsigned long long *__restrict__ counts)
{
  const long long items = n_words * 47;
  unsigned nerr = 0;
  for (long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x; i < items; i += (long long)gridDim.x * Q_THREADS) {
    const long long w = i / 47; const int p0 = (int)(i - w * 47) * 4;
    const unsigned got = *reinterpret_cast<const unsigned *>(rs_out + w * 188 + p0);      // (188 = 4 x 47: a word's data bytes are whole dwords)
    unsigned was = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int p = p0 + k;
      const long long src = (w - 11 + p % 12) * 204 + p;
      const unsigned b = (src >= 0 && src < n_vit) ? vit[src] : 0u;
      was |= b << (8 * k);
    }
    nerr += (unsigned)__builtin_popcount(got ^ was);
  }
  nerr = q_wave_sum(nerr);
  if ((threadIdx.x & 63) == 0 && nerr) atomicAdd(&counts[0], (unsigned long long)nerr);
}

}  // namespace dvbt
