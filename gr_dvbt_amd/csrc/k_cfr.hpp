// k_cfr.hpp -- crest-factor reduction by iterative clipping and filtering, one workgroup per OFDM symbol (include/dvbt_hip.h, dvbt_cfr_*).
//
// The current spectrum X (X0 wherever the filter holds the error back) and the sum over the oversampling phases live in registers: thread t owns the
// bins t + j FFT_THREADS, j < N / FFT_THREADS (4 at 2k, 16 at 8k).  The one LDS image of k_fft.hpp carries every transform: 2 per phase, 1 in front and 1
// behind.  A transform leaves bin k at fft_pos_of_bin(k), so a thread picks its bins (or, behind an inverse transform, its samples) up from there and puts
// them down in natural order for the next one; the barrier between the two is the only cost of the digit reversal.  The inverse goes through the swap
// identity of ifft_items_kernel.  Nothing is written to the output before the symbol's last transform, and the input is not read after it: in == out is
// safe.
#pragma once
#include "k_fft.hpp"

namespace dvbt {

enum { CFR_ACC_SYMBOLS = 0, CFR_ACC_CLIPPED, CFR_ACC_NONFINITE, CFR_ACC_OVER, CFR_ACC_PEAK /* a float's bit pattern, zero-extended */, CFR_ACC_WORDS = 8 };
constexpr size_t CFR_LDS_EXTRA = 16;                            // behind the FFT workspace: samples over, the peak's bits (first iteration)

struct CfrArgs {
  int G, iterations, os, phase0;                                // prefix length; (first_symbol + symbols so far) mod 4: the scattered-pilot phase of the call's first symbol
  float A, A2;                                                  // the threshold and its square, both float32
  const unsigned char *free_bins;                               // [4][N]: 1 where the filter lets the clipping error through, by scattered-pilot phase and bin
  unsigned long long *acc;                                      // [CFR_ACC_WORDS]
};

// Between the rounds of an unrolled loop over a thread's 16 bins: the scheduler would otherwise interleave 16 sine / cosine or division sequences, whose
// temporaries on top of X and C do not fit the 256 registers a wave of a 512-thread workgroup has
#define CFR_ONE_AT_A_TIME __builtin_amdgcn_sched_barrier(0)

// The thread's index as a value the compiler knows nothing about.  Every stretch of the kernel -- each transform, each round over the 16 bins -- addresses
// LDS and memory from the same index, and the compiler would keep all those addresses (well over 64 registers) from the first use to the last across the
// whole symbol; recomputing them where they are used is a few integer operations.
__device__ __forceinline__ int cfr_fresh(int v) { asm volatile("" : "+v"(v)); return v; }

__device__ __forceinline__ bool cfr_nonfinite(float2 v)
{
  return (__float_as_uint(v.x) & 0x7f800000u) == 0x7f800000u || (__float_as_uint(v.y) & 0x7f800000u) == 0x7f800000u;
}

// e^{2 pi i m / M}, M a power of two, |m| < 2^22: the argument 2 m / M of sincospi is exact
__device__ __forceinline__ float2 cfr_rot(int m, float two_over_m)
{
  float sn, cs;
  sincospif((float)m * two_over_m, &sn, &cs);
  return make_float2(cs, sn);
}

__device__ __forceinline__ void cfr_copy(const float2 *sin, float2 *sout, int n, int tid)
{
  if (sin == sout) return;
  for (int i = tid; i < n; i += FFT_THREADS) sout[i] = sin[i];
}

// a symbol that went through a first iteration: its counts, from what the workgroup left in LDS
__device__ __forceinline__ void cfr_count(unsigned long long *acc, const unsigned *red, int tid)
{
  if (tid != 0) return;
  const unsigned n_over = red[0];
  atomicAdd(acc + CFR_ACC_SYMBOLS, 1ull);
  atomicMax(acc + CFR_ACC_PEAK, (unsigned long long)red[1]);
  if (n_over) { atomicAdd(acc + CFR_ACC_CLIPPED, 1ull); atomicAdd(acc + CFR_ACC_OVER, (unsigned long long)n_over); }
}

// in and out may be the same buffer (no __restrict__)
template <int N>
__global__ __launch_bounds__(FFT_THREADS) void cfr_kernel(const float2 *in, float2 *out, int nsym, const float2 *__restrict__ tw, CfrArgs a)
{
  static_assert(N % FFT_THREADS == 0, "every thread owns N / FFT_THREADS bins");
  constexpr int NPT = N / FFT_THREADS;
  constexpr float INV_N = 1.0f / (float)N;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s >= nsym) return;
  const FftWork w = fft_work(smem_raw, N);
  unsigned *const red = reinterpret_cast<unsigned *>(w.end);
  const size_t base = (size_t)s * (size_t)(a.G + N);
  const float2 *const sin = in + base;
  float2 *const sout = out + base;

  fft_work_fill(w, N, tw, tid);
  if (tid < 2) red[tid] = 0;
  int bad = 0;
  for (int g = tid; g < a.G; g += FFT_THREADS) bad |= cfr_nonfinite(sin[g]);
#pragma unroll
  for (int j = 0; j < NPT; j++) {
    const int n = tid + j * FFT_THREADS;
    const float2 v = sin[a.G + n];
    bad |= cfr_nonfinite(v);
    w.x[fpad(n)] = v;
  }
  const int any_bad = __syncthreads_or(bad);
  if (any_bad || a.iterations == 0) {                           // (uniform over the workgroup)
    cfr_copy(sin, sout, a.G + N, tid);
    if (tid == 0) {
      atomicAdd(a.acc + CFR_ACC_SYMBOLS, 1ull);
      if (any_bad) atomicAdd(a.acc + CFR_ACC_NONFINITE, 1ull);
    }
    return;
  }

  fft_dif_lds(w, N, cfr_fresh(tid));
  float2 X[NPT], C[NPT];
  unsigned free_mask = 0;
  const unsigned char *const fb = a.free_bins + (size_t)((a.phase0 + s) & 3) * N;
#pragma unroll
  for (int j = 0; j < NPT; j++) {
    const int k = tid + j * FFT_THREADS;
    X[j] = w.x[fpad(fft_pos_of_bin(k, N))];
    free_mask |= (unsigned)fb[k] << j;
  }
  __syncthreads();                                              // every bin is read before the image is written again

  const float two_over_m = 2.0f / (float)(a.os * N), inv_os = 1.0f / (float)a.os;
  for (int it = 0; it < a.iterations; it++) {
#pragma unroll
    for (int j = 0; j < NPT; j++) C[j] = make_float2(0.f, 0.f);
    for (int p = 0; p < a.os; p++) {
      // phase p of X: the inverse transform of X r_p
#pragma unroll
      for (int j = 0; j < NPT; j++) {
        const int k = cfr_fresh(tid) + j * FFT_THREADS, kap = k < N / 2 ? k : k - N;
        w.x[fpad(k)] = cswap(p ? cmul(X[j], cfr_rot(kap * p, two_over_m)) : X[j]);
        CFR_ONE_AT_A_TIME;
      }
      __syncthreads();
      fft_dif_lds(w, N, cfr_fresh(tid));
      // clip
      float2 c[NPT];
      unsigned over = 0;
      float peak = 0.f;
#pragma unroll
      for (int j = 0; j < NPT; j++) {
        const int n = cfr_fresh(tid) + j * FFT_THREADS;
        const float2 v = w.x[fpad(fft_pos_of_bin(n, N))];
        float2 x = make_float2(v.y * INV_N, v.x * INV_N);
        const float pw = x.x * x.x + x.y * x.y;
        peak = fmaxf(peak, pw);
        if (pw > a.A2) {
          const float gain = a.A / sqrtf(pw);                   // division and square root are correctly rounded in this build
          x.x *= gain; x.y *= gain;
          over++;
        }
        c[j] = x;
        CFR_ONE_AT_A_TIME;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NPT; j++) w.x[fpad(tid + j * FFT_THREADS)] = c[j];
      if (it == 0) {
        if (over) atomicAdd(&red[0], over);
        atomicMax(&red[1], __float_as_uint(peak));              // non-negative floats order as their bit patterns
      }
      __syncthreads();
      fft_dif_lds(w, N, cfr_fresh(tid));
#pragma unroll
      for (int j = 0; j < NPT; j++) {
        if (!((free_mask >> j) & 1)) continue;
        const int k = cfr_fresh(tid) + j * FFT_THREADS, kap = k < N / 2 ? k : k - N;
        const float2 v = w.x[fpad(fft_pos_of_bin(k, N))];
        C[j] = cadd(C[j], p ? cmulc(v, cfr_rot(kap * p, two_over_m)) : v);      // (r_p again: 32 registers are worth more than 16 sines)
        CFR_ONE_AT_A_TIME;
      }
      __syncthreads();
    }
    if (it == 0 && red[0] == 0) {                               // (behind the phase loop's last barrier; uniform): nothing to clip
      cfr_copy(sin, sout, a.G + N, tid);
      cfr_count(a.acc, red, tid);
      return;
    }
    // filter: X = X0 + E is C / os where the error may pass and X0, which X still holds, elsewhere
#pragma unroll
    for (int j = 0; j < NPT; j++)
      if ((free_mask >> j) & 1) X[j] = make_float2(C[j].x * inv_os, C[j].y * inv_os);
  }

#pragma unroll
  for (int j = 0; j < NPT; j++) w.x[fpad(tid + j * FFT_THREADS)] = cswap(X[j]);
  __syncthreads();
  fft_dif_lds(w, N, cfr_fresh(tid));
#pragma unroll
  for (int j = 0; j < NPT; j++) {
    const int n = cfr_fresh(tid) + j * FFT_THREADS;
    const float2 v = w.x[fpad(fft_pos_of_bin(n, N))];
    const float2 y = make_float2(v.y * INV_N, v.x * INV_N);
    sout[a.G + n] = y;
    if (n >= N - a.G) sout[n - (N - a.G)] = y;                  // the cyclic prefix
  }
  cfr_count(a.acc, red, tid);
}

}  // namespace dvbt
