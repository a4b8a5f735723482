// k_scan.hpp -- the signal scanner's kernels (dvbt_scan.inc): the cyclic-prefix correlation of a complex64 stream at the lags 2048 and 8192, folded at the
// eight symbol lengths a DVB-T signal can have, accumulated in one pass.
//
// Hypothesis h = 4 mode + guard: N = 2048 or 8192, G = N / 32, / 16, / 8, / 4, S = N + G.  Symbol j of a hypothesis is the stream's samples [j S, j S + S),
// bin m of it is sample n = j S + m, and its terms are, with a = x[n] and b = x[n + N], each operation one rounded float operation (the library is built
// with -ffp-contract=off):
//   p.re = (a.re b.re) + (a.im b.im)        p.im = (a.im b.re) - (a.re b.im)        e = ((a.re a.re) + (a.im a.im)) + ((b.re b.re) + (b.im b.im))
// Everything that is summed in floating point is summed in an order fixed by the STREAM, never by the call (k_spectrum.hpp's rule): SCAN_GROUP consecutive
// symbols, [16 g, 16 g + 16) in the hypothesis' own numbering, are one group; one thread owns one bin of one group and adds the group's terms in ascending
// j into three float accumulators that start from +0.  A closed group is stored as one slab of 3 S floats (re, im, e: S each) and scan_fold_kernel adds
// the launch's slabs in ascending group order into 3 S doubles.  A group that a call leaves open is stored as it stands and the next call's threads start
// from it.  No float atomics; the one atomic counts non-finite samples, an integer.
#pragma once
#include <hip/hip_runtime.h>

namespace dvbt {

constexpr int SCAN_HYPS = 8;
constexpr int SCAN_GROUP = 16;                     // symbols per slab
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_HIST = 10240 + 8192;            // samples a later call can still need: fewer than N + S behind the newest one
constexpr int SCAN_BINS = 45760;                   // sum of S over the hypotheses

__host__ __device__ inline int scan_N(int h) { return (h >> 2) ? 8192 : 2048; }
__host__ __device__ inline int scan_G(int h) { return scan_N(h) >> (5 - (h & 3)); }
__host__ __device__ inline int scan_S(int h) { return scan_N(h) + scan_G(h); }
// where hypothesis h starts in an array laid out by bins: the S of the hypotheses before it
inline int scan_off(int h) { int o = 0; for (int i = 0; i < h; i++) o += scan_S(i); return o; }

struct ScanArgs {
  int N, S;
  long long j0, j1;                                // the call completes symbols [j0, j1) of this hypothesis
  long long pos0;                                  // stream index of the call's first input sample
  long long hbase;                                 // stream index of the carried history's first sample
};

__device__ __forceinline__ float2 scan_sample(const float2 *__restrict__ in, const float2 *__restrict__ hist, long long i, long long pos0, long long hbase)
{
  return i < pos0 ? hist[i - hbase] : in[i - pos0];
}

// One thread per bin (blockIdx.x tiles the S bins) of group g_first + blockIdx.y.
//   in        the call's input; hist: the carried samples [hbase, pos0)
//   open_in   the hypothesis' open group from the previous call, 3 S floats (read where j0 is inside a group)
//   open_out  where a group that this call leaves open is stored (another buffer than open_in: when the call spans groups, the thread that writes a bin
//             is not the one that reads it)
//   slabs     [gridDim.y][3 S] floats: the closed groups of this launch
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(const float2 *__restrict__ in, const float2 *__restrict__ hist, ScanArgs a, long long g_first,
                                                            const float *__restrict__ open_in, float *__restrict__ open_out, float *__restrict__ slabs)
{
  const int m = blockIdx.x * SCAN_THREADS + threadIdx.x, S = a.S;
  if (m >= S) return;
  const long long g = g_first + blockIdx.y;
  const long long ka = a.j0 > g * SCAN_GROUP ? a.j0 : g * SCAN_GROUP, kb = a.j1 < (g + 1) * SCAN_GROUP ? a.j1 : (g + 1) * SCAN_GROUP;
  const bool from_open = (ka % SCAN_GROUP) != 0, to_open = (kb % SCAN_GROUP) != 0;
  float re = 0.f, im = 0.f, en = 0.f;
  if (from_open) { re = open_in[m]; im = open_in[S + m]; en = open_in[2 * S + m]; }
  long long j = ka;
  if (ka * S >= a.pos0) {                          // (uniform) the group lies in this call's input: eight symbols' loads in flight, the additions in order
    const float2 *__restrict__ p = in + (ka * S + m - a.pos0);
    for (; j + 8 <= kb; j += 8, p += 8 * (size_t)S) {
      float2 x[8], y[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { x[u] = p[(size_t)u * S]; y[u] = p[(size_t)u * S + a.N]; }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        re = re + (x[u].x * y[u].x + x[u].y * y[u].y);
        im = im + (x[u].y * y[u].x - x[u].x * y[u].y);
        en = en + ((x[u].x * x[u].x + x[u].y * x[u].y) + (y[u].x * y[u].x + y[u].y * y[u].y));
      }
    }
  }
  for (; j < kb; j++) {
    const long long n = j * S + m;
    const float2 x = scan_sample(in, hist, n, a.pos0, a.hbase), y = scan_sample(in, hist, n + a.N, a.pos0, a.hbase);
    re = re + (x.x * y.x + x.y * y.y);
    im = im + (x.y * y.x - x.x * y.y);
    en = en + ((x.x * x.x + x.y * x.y) + (y.x * y.x + y.y * y.y));
  }
  float *const dst = to_open ? open_out : slabs + (size_t)blockIdx.y * 3 * S;
  dst[m] = re; dst[S + m] = im; dst[2 * S + m] = en;
}

// acc[e] += slab_0[e] + slab_1[e] + ... in ascending order, one thread per element of the 3 S
__global__ __launch_bounds__(SCAN_THREADS) void scan_fold_kernel(const float *__restrict__ slabs, int len, int nslabs, double *__restrict__ acc)
{
  const int e = blockIdx.x * SCAN_THREADS + threadIdx.x;
  if (e >= len) return;
  double s = acc[e];
  int q = 0;
  for (; q + 8 <= nslabs; q += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = slabs[(size_t)(q + u) * len + e];
#pragma unroll
    for (int u = 0; u < 8; u++) s += (double)v[u];
  }
  for (; q < nslabs; q++) s += (double)slabs[(size_t)q * len + e];
  acc[e] = s;
}

// the samples of the call that are not finite (either part inf or NaN), added to *count: one 64-bit integer atomic per wave that found any
__global__ __launch_bounds__(SCAN_THREADS) void scan_count_kernel(const float2 *__restrict__ in, long long n, unsigned long long *__restrict__ count)
{
  unsigned c = 0u;
  for (long long i = (long long)blockIdx.x * SCAN_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SCAN_THREADS) {
    const float2 v = in[i];
    const bool bad = (__float_as_uint(v.x) & 0x7f800000u) == 0x7f800000u || (__float_as_uint(v.y) & 0x7f800000u) == 0x7f800000u;
    c += bad ? 1u : 0u;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

// the samples [first, first + cnt) of the stream into next[0, cnt): what the next call needs of this one and of the history before it
__global__ __launch_bounds__(SCAN_THREADS) void scan_carry_kernel(const float2 *__restrict__ in, const float2 *__restrict__ hist, long long pos0,
                                                                  long long hbase, long long first, int cnt, float2 *__restrict__ next)
{
  const int j = blockIdx.x * SCAN_THREADS + threadIdx.x;
  if (j >= cnt) return;
  next[j] = scan_sample(in, hist, first + j, pos0, hbase);
}

}  // namespace dvbt
