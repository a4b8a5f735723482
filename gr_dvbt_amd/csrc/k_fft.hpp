// k_fft.hpp -- the generic FFT of one workgroup in LDS, and everything its callers have to agree on: the padded image, the two-level twiddle table behind
// it, the dynamic LDS a launch needs, where bin k stands after the transform.  Six kernels run it: fft_items_kernel and ifft_items_kernel here (the dvbt_fft
// block, both directions), derot_fft_kernel (k_frontend.hpp), tx_symbol_kernel (k_tx.hpp), spectrum_kernel (k_spectrum.hpp) and sounder_profile_kernel
// (k_sounder.hpp).  symbol8k_kernel and symbol2k_kernel have transforms of their own.
//
// The workspace, carved from the front of a kernel's dynamic LDS by fft_work():
//   x     [N + N / 32]       the padded image: element a at x[fpad(a)]
//   tw_c  [max(N / 128, 1)]  W_N^(128 i)
//   tw_f  [128]              W_N^t, t < 128 (t < N where N < 128)
//   end                      the first byte behind them: what else a kernel keeps in dynamic LDS starts here
// fft_lds_bytes(N) is its size.  A kernel fills the tables once (fft_work_fill), writes its N points in natural order, passes a barrier and calls
// fft_dif_lds; bin k is then at x[fpad(fft_pos_of_bin(k, N))].  tests/test_fft_index_host.py pins the index arithmetic on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace dvbt {

#ifndef DVBT_FFT_THREADS
#define DVBT_FFT_THREADS 512
#endif
constexpr int FFT_THREADS = DVBT_FFT_THREADS;   // workgroup size of the FFT kernels (a build-time experiment knob)

// ---------------------------------------------------------------- the arithmetic of the layout: host and device
// LDS image of a symbol: one float2 of padding after every 32 keeps the stride-4/16/64 accesses of the
// late radix-4 stages conflict-free (bank = float2 index mod 32 for ds_read_b64)
__host__ __device__ __forceinline__ int fpad(int a) { return a + (a >> 5); }

// LDS position that holds bin k after fft_dif_lds: digit reversal over the pass radices (16.. then 4 and/or 2)
__host__ __device__ __forceinline__ int fft_pos_of_bin(int k, int N)
{
  int L = N, p = 0;
  while (L >= 16) { L >>= 4; p += (k & 15) * L; k >>= 4; }
  if (L >= 4) { L >>= 2; p += (k & 3) * L; k >>= 2; }
  if (L == 2) p += k & 1;
  return p;
}

// entries of the coarse twiddle table: one per 128 twiddles, and one where N < 128
__host__ __device__ constexpr int fft_coarse(int N) { return N >= 128 ? N / 128 : 1; }
// dynamic LDS of the workspace: the padded image, the coarse table, 128 fine entries
__host__ __device__ constexpr size_t fft_lds_bytes(int N) { return (size_t)(N + N / 32 + fft_coarse(N) + 128) * 8; }
static_assert(fft_lds_bytes(64) == 1560 && fft_lds_bytes(128) == 2088 && fft_lds_bytes(1024) == 9536, "the FFT workspace's size");
static_assert(fft_lds_bytes(2048) == 18048 && fft_lds_bytes(4096) == 35072 && fft_lds_bytes(8192) == 69120, "the FFT workspace's size");

#ifdef __HIPCC__
// ---------------------------------------------------------------- the device side (a plain C++ compiler takes the arithmetic above alone: tests/host/fft_index_host.cpp)
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a*conj(b)
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cswap(float2 a) { return make_float2(a.y, a.x); }

// passed by value: four pointers that live in registers (by reference the compiler addresses the image differently in the radix-16 passes)
struct FftWork { float2 *x, *tw_c, *tw_f; unsigned char *end; };

__device__ __forceinline__ FftWork fft_work(unsigned char *smem, int N)
{
  const int nc = fft_coarse(N);
  FftWork w;
  w.x = reinterpret_cast<float2 *>(smem);
  w.tw_c = w.x + (N + N / 32);
  w.tw_f = w.tw_c + nc;
  w.end = reinterpret_cast<unsigned char *>(w.tw_f + 128);
  return w;
}

// the two tables out of the global one, tw[t] = W_N^t, t < N (FftPlan builds it); the caller's barrier in front of fft_dif_lds covers them
__device__ __forceinline__ void fft_work_fill(FftWork w, int N, const float2 *__restrict__ tw, int tid)
{
  const int nc = fft_coarse(N);
  for (int i = tid; i < nc; i += FFT_THREADS) w.tw_c[i] = tw[i * 128 < N ? i * 128 : 0];
  if (tid < 128 && tid < N) w.tw_f[tid] = tw[tid];
}

// twiddle W_N^t from a two-level table held in LDS: coarse[t >> 7] * fine[t & 127] (one complex multiply instead of
// an L2 round trip per twiddle; relative error ~1.2e-7)
__device__ __forceinline__ float2 twid(const float2 *coarse, const float2 *fine, int t) { return cmul(coarse[t >> 7], fine[t & 127]); }

// forward radix-4 butterfly: y_k = sum_j a_j (-i)^(jk)
__device__ __forceinline__ void bfly4(float2 a0, float2 a1, float2 a2, float2 a3, float2 &y0, float2 &y1, float2 &y2, float2 &y3)
{
  const float2 s02 = cadd(a0, a2), d02 = csub(a0, a2), s13 = cadd(a1, a3), d13 = csub(a1, a3);
  y0 = cadd(s02, s13); y2 = csub(s02, s13);
  y1 = make_float2(d02.x + d13.y, d02.y - d13.x);               // d02 - i*d13
  y3 = make_float2(d02.x - d13.y, d02.y + d13.x);               // d02 + i*d13
}

// 16-point forward DFT in registers (two radix-4 levels): a[j], j = time index, becomes A[k], k = frequency index
__device__ __forceinline__ void dft16(float2 (&a)[16])
{
  // W16^m = exp(-2 pi i m / 16), m = 0..9 (products r'*k1 with r',k1 <= 3)
  const float c1 = 0.92387953251128674f, s1 = 0.38268343236508977f, h = 0.70710678118654752f;
  const float2 w16[10] = {{1.f, 0.f}, {c1, -s1}, {h, -h}, {s1, -c1}, {0.f, -1.f}, {-s1, -c1}, {-h, -h}, {-c1, -s1}, {-1.f, 0.f}, {-c1, s1}};
  float2 t[16];
#pragma unroll
  for (int rp = 0; rp < 4; rp++) {                              // level 1: span 16
    float2 y0, y1, y2, y3;
    bfly4(a[rp], a[rp + 4], a[rp + 8], a[rp + 12], y0, y1, y2, y3);
    t[0 * 4 + rp] = y0;
    t[1 * 4 + rp] = rp ? cmul(y1, w16[rp]) : y1;
    t[2 * 4 + rp] = rp ? cmul(y2, w16[2 * rp]) : y2;
    t[3 * 4 + rp] = rp ? cmul(y3, w16[3 * rp]) : y3;
  }
#pragma unroll
  for (int k1 = 0; k1 < 4; k1++) {                              // level 2: span 4 -> A[k1 + 4*k2]
    float2 y0, y1, y2, y3;
    bfly4(t[k1 * 4], t[k1 * 4 + 1], t[k1 * 4 + 2], t[k1 * 4 + 3], y0, y1, y2, y3);
    a[k1] = y0; a[k1 + 4] = y1; a[k1 + 8] = y2; a[k1 + 12] = y3;
  }
}
// a[k] *= w1^k, k = 1..15: the powers by products, at most 4 multiplications deep
__device__ __forceinline__ void twiddle16(float2 (&a)[16], float2 w1)
{
  float2 w[16];
  w[1] = w1;
  w[2] = cmul(w[1], w[1]); w[3] = cmul(w[2], w[1]); w[4] = cmul(w[2], w[2]); w[5] = cmul(w[4], w[1]); w[6] = cmul(w[3], w[3]);
  w[7] = cmul(w[4], w[3]); w[8] = cmul(w[4], w[4]); w[9] = cmul(w[8], w[1]); w[10] = cmul(w[5], w[5]); w[11] = cmul(w[8], w[3]);
  w[12] = cmul(w[6], w[6]); w[13] = cmul(w[8], w[5]); w[14] = cmul(w[7], w[7]); w[15] = cmul(w[8], w[7]);
#pragma unroll
  for (int k = 1; k < 16; k++) a[k] = cmul(a[k], w[k]);
}

// In-place decimation-in-frequency FFT of the padded LDS image w.x (N points, natural order in, digit-reversed out: bin k at fft_pos_of_bin(k, N)).
// Radix-16 passes with the 16-point transform held in registers (two radix-4 levels), then a radix-4 and/or radix-2 tail: 8192 = 16.16.16.2,
// 2048 = 16.16.4.2.  One __syncthreads per pass; the caller's barrier stands between its writes to the workspace and the first pass.
__device__ __forceinline__ void fft_dif_lds(FftWork w, int N, int tid)
{
  float2 *const x = w.x;
  const float2 *const tw_c = w.tw_c, *const tw_f = w.tw_f;
  int L = N;
  while (L >= 16) {
    const int Q = L >> 4, tstep = N / L, nblk = (N >> 4) / Q;
    for (int bf = tid; bf < (N >> 4); bf += FFT_THREADS) {
      // butterfly bf = (block, r): consecutive lanes take consecutive r (conflict-free LDS columns); when only two r exist
      // (last radix-16 pass of 8k) consecutive lanes take consecutive blocks instead (stride 33 in the padded image).
      const int r = Q <= 2 ? bf / nblk : bf % Q, base = (Q <= 2 ? bf % nblk : bf / Q) * L + r;
      // padded address of element base + j Q: fpad is affine in j here (base % 32 = r < Q for Q < 32, and j Q % 32 = 0 otherwise)
      const int pb = fpad(base);
      float2 a[16];
#pragma unroll
      for (int j = 0; j < 16; j++) a[j] = x[pb + j * Q + ((j * Q) >> 5)];
      dft16(a);
      twiddle16(a, twid(tw_c, tw_f, r * tstep));       // inter-pass twiddles W^(r k tstep), k = 1..15
#pragma unroll
      for (int k = 0; k < 16; k++) x[pb + k * Q + ((k * Q) >> 5)] = a[k];
    }
    __syncthreads();
    L = Q;
  }
  if (L >= 4) {
    const int Q = L >> 2, tstep = N / L;
    for (int bf = tid; bf < (N >> 2); bf += FFT_THREADS) {
      const int r = bf % Q, base = (bf / Q) * L + r;
      const int i0 = fpad(base), i1 = fpad(base + Q), i2 = fpad(base + 2 * Q), i3 = fpad(base + 3 * Q);
      float2 y0, y1, y2, y3;
      bfly4(x[i0], x[i1], x[i2], x[i3], y0, y1, y2, y3);
      x[i0] = y0;
      if (r == 0) { x[i1] = y1; x[i2] = y2; x[i3] = y3; }
      else { x[i1] = cmul(y1, twid(tw_c, tw_f, r * tstep)); x[i2] = cmul(y2, twid(tw_c, tw_f, 2 * r * tstep)); x[i3] = cmul(y3, twid(tw_c, tw_f, 3 * r * tstep)); }
    }
    __syncthreads();
    L = Q;
  }
  if (L == 2) {
    for (int bf = tid; bf < (N >> 1); bf += FFT_THREADS) {
      const int j0 = fpad(2 * bf), j1 = fpad(2 * bf + 1);
      const float2 a0 = x[j0], a1 = x[j1];
      x[j0] = cadd(a0, a1); x[j1] = csub(a0, a1);
    }
    __syncthreads();
  }
}

// bin b of the shifted spectrum after fft_dif_lds: X[(b - N/2) mod N], as gr::fft::fft_vcc(forward, shift=True) writes out[b]
__device__ __forceinline__ float2 fft_shifted_bin(FftWork w, int b, int N) { return w.x[fpad(fft_pos_of_bin((b + (N >> 1)) & (N - 1), N))]; }

// ---------------------------------------------------------------- the dvbt_fft block: plain items, one workgroup each
// forward (the standalone A2 block: items already CP-stripped): out[b] = X[(b - N/2) mod N]
__global__ __launch_bounds__(FFT_THREADS) void fft_items_kernel(const float2 *__restrict__ in, int N, int nitems, const float2 *__restrict__ tw,
                                                                float2 *__restrict__ out)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s >= nitems) return;
  const FftWork w = fft_work(smem_raw, N);
  fft_work_fill(w, N, tw, tid);
  for (int n = tid; n < N; n += FFT_THREADS) w.x[fpad(n)] = in[(size_t)s * N + n];
  __syncthreads();
  fft_dif_lds(w, N, tid);
  for (int b = tid; b < N; b += FFT_THREADS) out[(size_t)s * N + b] = fft_shifted_bin(w, b, N);
}

// the inverse shifted FFT (dvbt_fft with forward = 0: gr::fft::fft_vcc(reverse, shift=True) of the TX flowgraphs):
// out[t] = sum_k in[(k + N/2) mod N] e^{+2 pi i t k / N}, unnormalised.  The inverse DFT through the forward one:
// swap(FFT(swap(X))) = IFFT(X) (swap(z) = i conj(z)), exact in the swaps.
__global__ __launch_bounds__(FFT_THREADS) void ifft_items_kernel(const float2 *__restrict__ in, int N, int nitems, const float2 *__restrict__ tw,
                                                                 float2 *__restrict__ out)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s >= nitems) return;
  const FftWork w = fft_work(smem_raw, N);
  fft_work_fill(w, N, tw, tid);
  for (int b = tid; b < N; b += FFT_THREADS) w.x[fpad((b + (N >> 1)) & (N - 1))] = cswap(in[(size_t)s * N + b]);
  __syncthreads();
  fft_dif_lds(w, N, tid);
  for (int t = tid; t < N; t += FFT_THREADS) out[(size_t)s * N + t] = cswap(w.x[fpad(fft_pos_of_bin(t, N))]);
}
#endif  // __HIPCC__

}  // namespace dvbt
