// k_spectrum.hpp -- the spectrum analyser's kernels (dvbt_spectrum.inc): an averaged, windowed periodogram (Welch) and amplitude statistics of a complex64
// stream, accumulated in one pass.
//
// Segment k is the stream's samples [k hop, k hop + N).  Everything that is summed in floating point is summed in an order fixed by the STREAM, never by
// the call: SPEC_GROUP consecutive segments, [32 g, 32 g + 32) in the stream's numbering, are one group, summed by one workgroup in segment order into
// float accumulators in registers (thread t owns bins t, t + 512, ...).  A closed group is stored as one slab of N floats and spectrum_fold_kernel adds
// the call's slabs in ascending group order into N doubles.  A group that a call leaves open is stored as it stands (the accumulators and the group's
// power sum) and the next call's first workgroup starts from it, so the additions run in the same order however the stream is cut.  No float
// atomics: their sums depend on arrival order.  The histogram and the peak are integers (64-bit atomic adds, an atomic max on the float's bits), which are
// order-free and so exact.
//
// Statistics cover the first `hop` samples of every complete segment, i.e. the samples [0, S hop) once each.  |x|^2 = fmaf(re, re, im im); its bits without
// the sign (only a NaN can carry one) shifted right by 20 are the histogram bin: 8 bins per octave over the whole float range, 2040.. = inf and NaN.
#pragma once
#include "k_fft.hpp"

namespace dvbt {

constexpr int SPEC_GROUP = 32;                     // segments per slab
constexpr int SPEC_HIST_BINS = 2048;
constexpr int SPEC_WAVES = FFT_THREADS / 64;

struct SpecArgs {
  int N, hop;
  long long s0, s1;                                // the call computes segments [s0, s1)
  long long pos0;                                  // stream index of the call's first input sample
  long long hbase;                                 // stream index of the carried history's first sample (s0 hop)
};

// the dynamic LDS of spectrum_kernel: the FFT's workspace, then the histogram's counters
inline size_t spec_lds(int N) { return fft_lds_bytes(N) + SPEC_HIST_BINS * sizeof(unsigned); }

// One workgroup per group of the launch: group g_first + blockIdx.x.  NB = max(N / FFT_THREADS, 1) accumulators per thread.
//   in        the call's input; hist: the carried samples [hbase, pos0)
//   open_in   the open group's state from the previous call (read where s0 is inside a group): its power sum (a double), then N floats
//   open_out  where a group that this call leaves open is stored (another buffer than open_in: other workgroups of this launch may still read that)
//   slabs     [gridDim.x][N] floats, psums [gridDim.x] doubles: the closed groups of this launch
// A segment's power sum is formed in a tree that depends on nothing but the thread numbering (a thread's samples in ascending order, xor-butterflies inside
// a wave, the waves in ascending order) and added to the group's, segment by segment.  Only the accumulators live across the transform: the per-thread
// index arithmetic starts from an opaque copy of the thread number in each phase, so that none of it is kept in registers from one segment to the next
// (with it the kernel needs more than the 128 registers that let two workgroups share a CU).
template <int NB>
__global__ __launch_bounds__(FFT_THREADS, 4) void spectrum_kernel(const float2 *__restrict__ in, const float2 *__restrict__ hist, const float *__restrict__ win,
                                                                  const float2 *__restrict__ tw, SpecArgs a, long long g_first,
                                                                  const double *__restrict__ open_in, double *__restrict__ open_out,
                                                                  float *__restrict__ slabs, double *__restrict__ psums,
                                                                  unsigned long long *__restrict__ hist64, unsigned *__restrict__ peak)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_w[SPEC_WAVES];
  __shared__ double s_gsum;
  __shared__ unsigned s_peak;
  const int N = a.N, hop = a.hop, tid = threadIdx.x;
  const FftWork fw = fft_work(smem_raw, N);
  float2 *const x = fw.x;
  unsigned *cnt = reinterpret_cast<unsigned *>(fw.end);
  fft_work_fill(fw, N, tw, tid);
  for (int i = tid; i < SPEC_HIST_BINS; i += FFT_THREADS) cnt[i] = 0u;

  const long long g = g_first + blockIdx.x;
  const long long ka = a.s0 > g * SPEC_GROUP ? a.s0 : g * SPEC_GROUP, kb = a.s1 < (g + 1) * SPEC_GROUP ? a.s1 : (g + 1) * SPEC_GROUP;
  const bool from_open = (ka % SPEC_GROUP) != 0, to_open = (kb % SPEC_GROUP) != 0;
  if (tid == 0) { s_peak = 0u; s_gsum = from_open ? open_in[0] : 0.0; }
  float acc[NB];
#pragma unroll
  for (int j = 0; j < NB; j++) acc[j] = 0.f;
  if (from_open) {
    const float *oa = reinterpret_cast<const float *>(open_in + 1);
#pragma unroll
    for (int j = 0; j < NB; j++) { const int b = tid + j * FFT_THREADS; if (b < N) acc[j] = oa[b]; }
  }
  __syncthreads();

  for (long long k = ka; k < kb; k++) {
    const long long i0 = k * hop;
    int t = tid;
    asm volatile("" : "+v"(t));
    double ps = 0.0;
    unsigned pm = 0u;
    for (int n = t; n < N; n += FFT_THREADS) {
      const long long i = i0 + n;
      const float2 v = i < a.pos0 ? hist[i - a.hbase] : in[i - a.pos0];
      if (n < hop) {
        const float p = fmaf(v.x, v.x, v.y * v.y);
        const unsigned bits = __float_as_uint(p) & 0x7fffffffu;
        atomicAdd(&cnt[bits >> 20], 1u);
        pm = bits > pm ? bits : pm;
        ps += (double)p;
      }
      const float w = win[n];
      x[fpad(n)] = make_float2(v.x * w, v.y * w);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      ps += __shfl_xor(ps, m, 64);
      const unsigned o = __shfl_xor(pm, m, 64);
      pm = o > pm ? o : pm;
    }
    if ((t & 63) == 0) { s_w[t >> 6] = ps; atomicMax(&s_peak, pm); }
    __syncthreads();
    if (t == 0) {                                  // before the transform's first barrier; s_w is written again behind its last
      double s = s_gsum;
      for (int w = 0; w < SPEC_WAVES; w++) s += s_w[w];
      s_gsum = s;
    }
    fft_dif_lds(fw, N, tid);                       // ends behind a barrier
    int u = tid, Nk = N;
    asm volatile("" : "+v"(u), "+s"(Nk));
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int b = u + j * FFT_THREADS;
      if (b < Nk) {
        const float2 X = fft_shifted_bin(fw, b, Nk);   // as dvbt_fft: bin b is X[(b - N/2) mod N]
        acc[j] = acc[j] + (X.x * X.x + X.y * X.y);
      }
    }
    __syncthreads();
  }

  float *dst = to_open ? reinterpret_cast<float *>(open_out + 1) : slabs + (size_t)blockIdx.x * N;
#pragma unroll
  for (int j = 0; j < NB; j++) { const int b = tid + j * FFT_THREADS; if (b < N) dst[b] = acc[j]; }
  if (tid == 0) {
    if (to_open) open_out[0] = s_gsum; else psums[blockIdx.x] = s_gsum;
    if (s_peak) atomicMax(peak, s_peak);
  }
  for (int i = tid; i < SPEC_HIST_BINS; i += FFT_THREADS) { const unsigned c = cnt[i]; if (c) atomicAdd(&hist64[i], (unsigned long long)c); }
}

// acc[b] += slab_0[b] + slab_1[b] + ... in ascending order, one thread per bin; thread N does the same for the groups' power sums
__global__ __launch_bounds__(256) void spectrum_fold_kernel(const float *__restrict__ slabs, const double *__restrict__ psums, int N, int nslabs,
                                                            double *__restrict__ acc, double *__restrict__ psum)
{
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < N) {
    double s = acc[b];
    int q = 0;
    for (; q + 8 <= nslabs; q += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = slabs[(size_t)(q + u) * N + b];
#pragma unroll
      for (int u = 0; u < 8; u++) s += (double)v[u];
    }
    for (; q < nslabs; q++) s += (double)slabs[(size_t)q * N + b];
    acc[b] = s;
  } else if (b == N) {
    double s = *psum;
    for (int q = 0; q < nslabs; q++) s += psums[q];
    *psum = s;
  }
}

// the samples [first, first + cnt) of the stream into next[0, cnt): what the next call needs of this one and of the history before it
__global__ __launch_bounds__(256) void spectrum_carry_kernel(const float2 *__restrict__ in, const float2 *__restrict__ hist, long long pos0, long long hbase,
                                                             long long first, int cnt, float2 *__restrict__ next)
{
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= cnt) return;
  const long long i = first + j;
  next[j] = i < pos0 ? hist[i - hbase] : in[i - pos0];
}

}  // namespace dvbt
