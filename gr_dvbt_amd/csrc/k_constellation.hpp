// k_constellation.hpp -- the constellation analyser's kernel (dvbt_constellation.inc): the I/Q density, the error cloud of every constellation point and the
// signal and error sums of every carrier, accumulated from rows of equalised cells in one pass.  include/dvbt_hip.h has the definitions.
//
// Everything that is summed is an integer: a cell's error vector is quantised once (con_axis: single float32 operations, __fmul_rn / __fsub_rn, so that no
// compiler setting can contract them) and every sum behind that is an integer add, which commutes: no order is kept anywhere, and the launch geometry is
// free.  A workgroup owns a tile of columns and a band of rows.  A thread keeps its two adjacent columns (16 bytes a row where rows allow it) over its rows
// and so owns their carrier sums in registers.  The density (G x G counters of 32 bits), the point counts (64 of 32 bits) and the point moments (5 x 64 of
// 64 bits, a moment's 64 points side by side so that they spread over the banks) are private to the workgroup in LDS and flushed with one 64-bit atomic
// per non-zero counter at the end, as spectrum_kernel does: on a clean signal every cell of the stream falls on 64 points and a few hundred bins, and
// global atomics would all meet on a few lines of L2.  A moment that a cell leaves unchanged (a zero) is not added.  A 32-bit counter holds what a
// workgroup can give it: the host keeps a workgroup's cells at or below CON_MAX_WG_CELLS.
#pragma once

namespace dvbt {

constexpr int CON_GRID = 128;                      // DVBT_CONSTELLATION_GRID
constexpr int CON_THREADS = 512;
constexpr int CON_UNROLL = 4;                      // rows in flight per thread
constexpr int CON_MAX_POINTS = 64;
constexpr long long CON_MAX_WG_CELLS = 1ll << 31;  // per workgroup: what an LDS counter of 32 bits holds, with room

struct ConArgs {
  int P;                                           // cells per row
  int alpha, H;                                    // the grid: levels alpha + 2 j, j < H
  float inv_d, bin_scale;                          // G / (2 S)
  int tx, ty;                                      // a workgroup: tx threads side by side (2 tx columns), ty rows at a time; tx ty <= CON_THREADS
  int band;                                        // rows per workgroup along y
  int nrows;
};

// where the accumulators lie in the handle's array of 64-bit words
__host__ __device__ inline size_t con_off_points() { return (size_t)CON_GRID * CON_GRID; }
__host__ __device__ inline size_t con_off_carriers() { return con_off_points() + (size_t)CON_MAX_POINTS * 6; }
__host__ __device__ inline size_t con_off_totals(int P) { return con_off_carriers() + (size_t)P * 3; }     // nonfinite, clipped
__host__ __device__ inline size_t con_words(int P) { return con_off_totals(P) + 2; }

// the dynamic LDS: the density's counters, the moments [5][64], the point counts [64]
__host__ __device__ inline size_t con_lds_mom() { return (size_t)CON_GRID * CON_GRID * sizeof(unsigned); }
__host__ __device__ inline size_t con_lds_pn() { return con_lds_mom() + (size_t)CON_MAX_POINTS * 5 * sizeof(unsigned long long); }
__host__ __device__ inline size_t con_lds() { return con_lds_pn() + (size_t)CON_MAX_POINTS * sizeof(unsigned); }

struct ConAxis { int q, idx, level, bin; bool nonfinite, clipped; };

// one component of one cell: the header's steps, each one float32 operation
__device__ __forceinline__ ConAxis con_axis(float x, const ConArgs &a)
{
  ConAxis o;
  const unsigned bits = __float_as_uint(x);
  const bool neg = (bits >> 31) != 0;
  o.nonfinite = (bits & 0x7f800000u) == 0x7f800000u;
  const float av = __uint_as_float(bits & 0x7fffffffu);
  const float u = __fmul_rn(av, a.inv_d);
  const float t = __fmul_rn(__fsub_rn(u, (float)(a.alpha - 1)), 0.5f);
  const int j = min(max((int)fminf(t, 8.0f), 0), a.H - 1);          // t < 1 ? 0 : t >= H ? H - 1 : (int)t, with a conversion that is always in range
  o.level = a.alpha + 2 * j;
  const float r = rintf(__fmul_rn(__fsub_rn(u, (float)o.level), 4096.0f));
  o.clipped = fabsf(r) > 32767.0f;
  const int q = (int)fminf(fmaxf(r, -32767.0f), 32767.0f);
  o.q = neg ? -q : q;
  o.idx = neg ? a.H - 1 - j : a.H + j;
  const float e = neg ? -u : u;
  o.bin = (int)fminf(fmaxf(floorf(__fmul_rn(e, a.bin_scale)), (float)(-CON_GRID / 2)), (float)(CON_GRID / 2 - 1)) + CON_GRID / 2;
  return o;
}

struct ConCarrier { unsigned n, signal; unsigned long long error; };

__device__ __forceinline__ void con_lds_add(unsigned long long *p, int v)
{
  if (v) atomicAdd(p, (unsigned long long)(long long)v);      // (two's complement: a signed sum in an unsigned word)
}

__device__ __forceinline__ void con_cell(float re, float im, const ConArgs &a, unsigned *cnt, unsigned long long *mom, unsigned *pn, unsigned *flags,
                                         ConCarrier &c)
{
  const ConAxis x = con_axis(re, a), y = con_axis(im, a);
  if (x.nonfinite || y.nonfinite) { atomicAdd(&flags[0], 1u); return; }
  if (x.clipped || y.clipped) atomicAdd(&flags[1], 1u);
  atomicAdd(&cnt[y.bin * CON_GRID + x.bin], 1u);
  const int p = y.idx * 2 * a.H + x.idx;
  unsigned long long *m = mom + p;
  const int qx = x.q, qy = y.q, xy = qx * qy, xx = qx * qx, yy = qy * qy;       // |q| <= 32767: the products fit 32 bits, two squares 31
  atomicAdd(&pn[p], 1u);
  con_lds_add(&m[0 * CON_MAX_POINTS], qx);
  con_lds_add(&m[1 * CON_MAX_POINTS], qy);
  con_lds_add(&m[2 * CON_MAX_POINTS], xy);
  con_lds_add(&m[3 * CON_MAX_POINTS], xx);
  con_lds_add(&m[4 * CON_MAX_POINTS], yy);
  c.n += 1u;
  c.signal += (unsigned)(x.level * x.level + y.level * y.level);
  c.error += (unsigned)(xx + yy);
}

// blockIdx.x: the tile of 2 tx columns; blockIdx.y: the band of rows [y band, (y + 1) band).  VEC: P is even and the rows are 16-byte aligned, so a thread
// reads its two cells in one load.  acc: the handle's 64-bit words (con_off_*).
template <bool VEC>
__global__ __launch_bounds__(CON_THREADS) void constellation_kernel(const float2 *__restrict__ rows, ConArgs a, unsigned long long *__restrict__ acc)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ unsigned s_flags[2];
  unsigned *cnt = reinterpret_cast<unsigned *>(smem_raw);
  unsigned long long *mom = reinterpret_cast<unsigned long long *>(smem_raw + con_lds_mom());
  unsigned *pn = reinterpret_cast<unsigned *>(smem_raw + con_lds_pn());
  const int tid = threadIdx.x;
  for (int i = tid; i < CON_GRID * CON_GRID; i += CON_THREADS) cnt[i] = 0u;
  for (int i = tid; i < CON_MAX_POINTS * 5; i += CON_THREADS) mom[i] = 0ull;
  if (tid < CON_MAX_POINTS) pn[tid] = 0u;
  if (tid < 2) s_flags[tid] = 0u;
  __syncthreads();

  const int lx = tid % a.tx, ly = tid / a.tx;
  const int c0 = ((int)blockIdx.x * a.tx + lx) * 2;
  const long long r0 = (long long)blockIdx.y * a.band;
  const long long r1 = r0 + a.band < a.nrows ? r0 + a.band : a.nrows;
  const bool have0 = ly < a.ty && c0 < a.P, have1 = have0 && c0 + 1 < a.P;
  ConCarrier k0 = {0u, 0u, 0ull}, k1 = {0u, 0u, 0ull};
  if (have0) {
    const float2 *p = rows + c0;
    long long r = r0 + ly;
    const long long step = a.ty;
    for (; r + (CON_UNROLL - 1) * step < r1; r += CON_UNROLL * step) {
      float4 v[CON_UNROLL];
#pragma unroll
      for (int u = 0; u < CON_UNROLL; u++) {
        const float2 *q = p + (r + u * step) * a.P;
        if (VEC) v[u] = *reinterpret_cast<const float4 *>(q);
        else { const float2 lo = q[0], hi = have1 ? q[1] : make_float2(0.f, 0.f); v[u] = make_float4(lo.x, lo.y, hi.x, hi.y); }
      }
#pragma unroll
      for (int u = 0; u < CON_UNROLL; u++) {
        con_cell(v[u].x, v[u].y, a, cnt, mom, pn, s_flags, k0);
        if (have1) con_cell(v[u].z, v[u].w, a, cnt, mom, pn, s_flags, k1);
      }
    }
    for (; r < r1; r += step) {
      const float2 *q = p + r * a.P;
      float4 v;
      if (VEC) v = *reinterpret_cast<const float4 *>(q);
      else { const float2 lo = q[0], hi = have1 ? q[1] : make_float2(0.f, 0.f); v = make_float4(lo.x, lo.y, hi.x, hi.y); }
      con_cell(v.x, v.y, a, cnt, mom, pn, s_flags, k0);
      if (have1) con_cell(v.z, v.w, a, cnt, mom, pn, s_flags, k1);
    }
    unsigned long long *car = acc + con_off_carriers() + (size_t)c0 * 3;
    if (k0.n) { atomicAdd(&car[0], (unsigned long long)k0.n); atomicAdd(&car[1], (unsigned long long)k0.signal); if (k0.error) atomicAdd(&car[2], k0.error); }
    if (k1.n) { atomicAdd(&car[3], (unsigned long long)k1.n); atomicAdd(&car[4], (unsigned long long)k1.signal); if (k1.error) atomicAdd(&car[5], k1.error); }
  }
  __syncthreads();
  for (int i = tid; i < CON_GRID * CON_GRID; i += CON_THREADS) { const unsigned c = cnt[i]; if (c) atomicAdd(&acc[i], (unsigned long long)c); }
  for (int i = tid; i < CON_MAX_POINTS * 5; i += CON_THREADS) {                  // moment i / 64 of point i % 64: the record's word 1 + i / 64
    const unsigned long long m = mom[i];
    if (m) atomicAdd(&acc[con_off_points() + (size_t)(i % CON_MAX_POINTS) * 6 + 1 + i / CON_MAX_POINTS], m);
  }
  if (tid < CON_MAX_POINTS && pn[tid]) atomicAdd(&acc[con_off_points() + (size_t)tid * 6], (unsigned long long)pn[tid]);
  if (tid < 2 && s_flags[tid]) atomicAdd(&acc[con_off_totals(a.P) + tid], (unsigned long long)s_flags[tid]);
}

}  // namespace dvbt
