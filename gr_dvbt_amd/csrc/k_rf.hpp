// k_rf.hpp -- the RF front-end block's kernel (dvbt_rf_*, csrc/dvbt_rf.inc): what the radio hardware on either side of a channel does to complex64 baseband.
//
//   u = x (1 + (|x|^2 / A^2)^p)^(-1/(2p))                       the power amplifier (Rapp AM/AM; the phase is untouched)
//   r = u cis(phi(n))    phi(n) = sum_m a_m sin(2 pi theta_m(n))   oscillator phase noise as a sum of tones; theta_m = top 32 bits of (ph_m + inc_m n mod 2^64)
//   v = mu r + nu conj(r)                                        the tuner's IQ imbalance
//   y = v + dc                                                   and its DC offset
//
// n is the sample's absolute index in the stream.  The block is memoryless: a sample's output bits are a function of (the parameters, n, x[n]) alone, so a
// stream cut into calls of any size gives the bytes of one call, and input and output may be one buffer.  A stage that is off is a uniform branch not taken.
//
// A workgroup owns RF_TILE samples; lane t works on the sample pairs at 2 t and 2 t + RF_TILE / 2 of the tile, each one 128-bit load and store where both
// samples lie in the call.  Pairs are counted from the output pointer's 16-byte boundary (`lead`), so the stores are aligned, and the loads are where the input
// has the output's parity (in place: always).  The tone table lives in the kernel arguments: every lane reads the same tone, so it arrives by scalar loads.
// The 64-bit phase of a lane's first sample is the workgroup's (scalar arithmetic) plus inc times the lane's offset; the other three are additions.
#pragma once
#include "k_channel.hpp"

namespace dvbt {

constexpr int RF_MAX_TONES = 32;
constexpr int RF_THREADS = 256;
constexpr int RF_TILE = 4 * RF_THREADS;                    // samples of a workgroup: two pairs per lane

struct RfArgs {
  int has_pa; float A, lg_a2, p, e;                        // lg_a2 = (float)(2 log2 A), e = (float)(-1 / (2 p))
  int n_tones; unsigned long long inc[RF_MAX_TONES], ph[RF_MAX_TONES]; float amp[RF_MAX_TONES];
  int has_iq; float mu_re, mu_im, nu_re, nu_im;
  int has_dc; float dc_re, dc_im;
};

// sin(2 pi p / 2^32): the nearest half turn comes off as an integer, the rest (|x| <= pi / 2) goes through the Taylor polynomial to x^13, whose first omitted
// term is 7e-10.  The low bits of p that a float cannot hold (6 of the remainder's 30) are rounded away: 5e-8 rad.
__device__ __forceinline__ float rf_sin_turns(uint32_t p)
{
  const uint32_t q = (p + 0x40000000u) >> 31;
  const int r = (int)(p - (q << 31));
  const float x = (float)r * 1.4629180792671596e-9f;      // 2 pi / 2^32
  const float z = x * x;
  float sp = __builtin_fmaf(z, 1.6059044e-10f, -2.5052108e-8f);
  sp = __builtin_fmaf(z, sp, 2.7557319e-6f); sp = __builtin_fmaf(z, sp, -1.9841270e-4f);
  sp = __builtin_fmaf(z, sp, 8.3333333e-3f); sp = __builtin_fmaf(z, sp, -1.6666667e-1f);
  const float sn = __builtin_fmaf(x * z, sp, x);
  return (q & 1) ? -sn : sn;
}

// Rapp AM/AM for every finite x.  The sample is scaled by a power of two (exactly) so that its larger component lies in [1/2, 1); with s = |x 2^-k|^2 in
// [1/4, 2) the amplifier's drive is L = log2(|x|^2 / A^2) = log2 s + 2 k - 2 log2 A, and with q = 2^(-p |L|) <= 1, h = (1 + q)^(-1/(2p)):
//   |x| <= A:  u = x h                                  (the definition)
//   |x| >  A:  u = x t^(-1/2) (1 + t^(-p))^(-1/(2p)) = (x 2^-k) h A / sqrt(s)     t = |x|^2 / A^2
// Nothing here grows with |x|: no intermediate overflows.  x = 0 takes the first form with k = 0, s = 0, L = -inf, q = 0, h = 1 and stays 0.  The two forms are
// one chain of instructions with two selects, so a wave whose lanes lie on both sides of A does not run both.
__device__ __forceinline__ float2 rf_pa(float2 x, const RfArgs &a)
{
  const int k = __builtin_amdgcn_frexp_expf(__builtin_fmaxf(__builtin_fabsf(x.x), __builtin_fabsf(x.y)));
  const float xr = __builtin_amdgcn_ldexpf(x.x, -k), xi = __builtin_amdgcn_ldexpf(x.y, -k);
  const float s = xr * xr + xi * xi;
  const float L = __builtin_amdgcn_logf(s) + ((float)(2 * k) - a.lg_a2);
  const float q = __builtin_amdgcn_exp2f(-a.p * __builtin_fabsf(L));
  const float h = __builtin_amdgcn_exp2f(a.e * __builtin_amdgcn_logf(1.0f + q));
  const bool above = L > 0.f;
  const float g = above ? h * a.A * __builtin_amdgcn_rsqf(s) : h;
  const int back = above ? 0 : k;
  return make_float2(__builtin_amdgcn_ldexpf(xr * g, back), __builtin_amdgcn_ldexpf(xi * g, back));
}

// What a lane's four samples go through behind their loads, side by side so that the four chains of arithmetic overlap: e[0], e[1] are the samples n, n + 1 and
// e[2], e[3] the samples n + RF_TILE / 2, n + RF_TILE / 2 + 1, where n = nb + off: nb is the same for the whole workgroup, off the lane's.  Each sample's
// arithmetic is its own: the same whatever its neighbours are and whichever way it was loaded.
__device__ __forceinline__ void rf_quad(float2 e[4], unsigned long long nb, uint32_t off, const RfArgs &a)
{
  if (a.has_pa) {
#pragma unroll
    for (int k = 0; k < 4; k++) e[k] = rf_pa(e[k], a);
  }
  if (a.n_tones > 0) {
    float phi[4] = {0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < a.n_tones; m++) {
      const unsigned long long inc = a.inc[m];
      const float am = a.amp[m];
      // ph + inc n mod 2^64 has the same bits however the product is cut: the workgroup's part is the same in every lane and is held in scalar registers
      // (the compiler would otherwise fold it back into one 64 x 64 product per lane), the lane's part is a 64 x 32 product
      const unsigned long long wg = a.ph[m] + inc * nb;
      const uint32_t wg_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(wg >> 32)), wg_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wg);
      const unsigned long long base = ((unsigned long long)wg_hi << 32) | (unsigned long long)wg_lo;      // (the builtin returns an int: widened unsigned)
      unsigned long long th[4];
      th[0] = base + inc * (unsigned long long)off;
      th[1] = th[0] + inc;
      th[2] = th[0] + inc * (unsigned long long)(RF_TILE / 2);
      th[3] = th[2] + inc;
#pragma unroll
      for (int k = 0; k < 4; k++) phi[k] = phi[k] + am * rf_sin_turns((uint32_t)(th[k] >> 32));
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      // |phi| <= sum a_m <= pi up to rounding: to turns of 2^-32, kept inside an int
      const float tu = __builtin_fminf(__builtin_fmaxf(phi[k] * 683565275.57643159f, -2147483648.f), 2147483520.f);
      float c, s;
      ch_cossin_turns((uint32_t)(int)__builtin_rintf(tu), c, s);
      e[k] = make_float2(c * e[k].x - s * e[k].y, c * e[k].y + s * e[k].x);
    }
  }
  if (a.has_iq) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float2 r = e[k];
      const float dr = a.mu_re * r.x - a.mu_im * r.y, di = a.mu_re * r.y + a.mu_im * r.x;              // mu r
      const float cr = a.nu_re * r.x + a.nu_im * r.y, ci = a.nu_im * r.x - a.nu_re * r.y;              // nu conj(r)
      e[k] = make_float2(dr + cr, di + ci);
    }
  }
  if (a.has_dc) {
#pragma unroll
    for (int k = 0; k < 4; k++) e[k] = make_float2(e[k].x + a.dc_re, e[k].y + a.dc_im);
  }
}

// Workgroup b owns the samples b RF_TILE - lead .. of the call (lead = 0 or 1: one where out is not 16-byte aligned, so that every pair's store is); in[0] is
// the stream's sample n0, the call has cnt samples.  A pair with one sample outside the call -- the first pair where lead = 1, the last one where the call
// ends inside it -- loads and stores the other alone; the missing one stands in as a copy of it.  in and out are the same buffer or do not overlap.
__global__ __launch_bounds__(RF_THREADS) void rf_kernel(const float2 *in, float2 *out, long long n0, long long cnt, int lead, RfArgs a)
{
  const uint32_t off = 2u * threadIdx.x;
  const long long j0 = (long long)blockIdx.x * RF_TILE - lead;        // the tile's first sample in the call; -1 in the first tile where lead = 1
  long long j[2]; bool v[4];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    j[h] = j0 + h * (RF_TILE / 2) + off;
    v[2 * h] = j[h] >= 0 && j[h] < cnt; v[2 * h + 1] = j[h] + 1 < cnt;                                // j + 1 >= 0 always
  }
  if (!(v[0] || v[1])) return;                                                                         // the first pair begins behind the call: so does the second
  float2 e[4];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    if (v[2 * h] && v[2 * h + 1]) { const ChPair q = *reinterpret_cast<const ChPair *>(in + j[h]); e[2 * h] = make_float2(q.v.x, q.v.y); e[2 * h + 1] = make_float2(q.v.z, q.v.w); }
    else if (v[2 * h]) e[2 * h] = e[2 * h + 1] = in[j[h]];
    else if (v[2 * h + 1]) e[2 * h] = e[2 * h + 1] = in[j[h] + 1];
    else e[2 * h] = e[2 * h + 1] = make_float2(0.f, 0.f);
  }
  rf_quad(e, (unsigned long long)(n0 + j0), off, a);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    if (v[2 * h] && v[2 * h + 1]) { ChPair q; q.v = ch_float4{e[2 * h].x, e[2 * h].y, e[2 * h + 1].x, e[2 * h + 1].y}; *reinterpret_cast<ChPair *>(out + j[h]) = q; }
    else if (v[2 * h]) out[j[h]] = e[2 * h];
    else if (v[2 * h + 1]) out[j[h] + 1] = e[2 * h + 1];
  }
}

}  // namespace dvbt
