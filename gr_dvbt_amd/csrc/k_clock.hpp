// k_clock.hpp -- the sample-clock offset block's kernel (dvbt_clock_*, csrc/dvbt_clock.inc): the stream as a receiver whose sample clock is off by some ppm
// sees it, by windowed-sinc interpolation.
//
//   y[m] = sum_{k = -(H-1)}^{H} h(k - f / 2^64) x[base + k]        h(a) = sinc(a) (0.54 + 0.46 cos(pi a / (H + 1)))        H = taps / 2
//
// base and f are the two words of the 128-bit integer position P(m) = P0 + m S (k_clock_math.hpp), m and the x index count from the stream's beginning: so an
// output is a function of m and of the taps samples around base alone, whatever call, workgroup or lane it falls into.  f == 0 is x[base] itself.
//
// Coefficients by direct evaluation, per output: sin(pi (k - phi)) = -(-1)^k sin(pi phi), so one sine serves every tap; the window's cosine comes by angle
// addition from the constants cos / sin(pi k / (H + 1)) (ClockArgs, made by the host in double) and one cos / sin(pi phi / (H + 1)); each tap costs one
// reciprocal.  The fraction enters as g = min(f, 2^64 - f), taken as an integer before it is converted: the tap next to the sampling instant (k = 0 for
// f < 1/2, k = 1 above) then has the argument -+g 2^-64 exactly and sin(pi g 2^-64) is evaluated from that float, so its ratio keeps its relative precision
// down to g = 1 and never becomes 0 / 0.  (ch_cossin_turns takes its angle in 2^-32 turns: what is left of a small g there is 0.)  Every other tap has
// |k - phi| >= 1/2.
//
// Loads: the inputs a workgroup's CLK_THREADS outputs need are consecutive -- at most CLK_THREADS (1 + 1e-3) + taps + 1 of them -- and are staged in LDS once,
// coalesced; lane t then reads tile[off_t + i] for tap i, stride 1 over the lanes but for the one place per 1e6 / ppm outputs where base skips or repeats.
// A sample in front of the call comes from the handle's history of the last CLK_HIST inputs, exactly as in k_channel.hpp, and the workgroup behind the
// compute workgroups writes the history the next call reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_clock_math.hpp"

namespace dvbt {

constexpr int CLK_THREADS = 256;
constexpr int CLK_MAX_TAPS = 64;
constexpr int clk_tile(int taps) { return CLK_THREADS + taps + 8; }   // off <= ceil(255 (1 + 1e-3)) + 1 = 257, so off + taps <= 257 + taps

struct ClockArgs {
  ClockStep c;
  float wc[CLK_MAX_TAPS], ws[CLK_MAX_TAPS];   // -(-1)^k 0.46 cos, -(-1)^k 0.46 sin of pi k / (H + 1) for tap i = k + H - 1
};

// sin x and cos x for |x| <= pi / 4: the polynomials of ch_cossin_turns
__device__ __forceinline__ void clk_cossin(float x, float &c, float &s)
{
  const float z = x * x;
  float sp = __builtin_fmaf(z, 2.7557319e-6f, -1.9841270e-4f);
  sp = __builtin_fmaf(z, sp, 8.3333333e-3f); sp = __builtin_fmaf(z, sp, -1.6666667e-1f);
  s = __builtin_fmaf(x * z, sp, x);
  float cp = __builtin_fmaf(z, -2.7557319e-7f, 2.4801587e-5f);
  cp = __builtin_fmaf(z, cp, -1.3888889e-3f); cp = __builtin_fmaf(z, cp, 4.1666667e-2f); cp = __builtin_fmaf(z, cp, -0.5f);
  c = __builtin_fmaf(z, cp, 1.0f);
}

// sin(pi g) for 0 < g <= 1/2, relative precision kept as g -> 0: below 1/4 the sine of pi g, above it the cosine of pi (1/2 - g) (the difference is exact)
__device__ __forceinline__ float clk_sinpi(float g)
{
  const bool low = g <= 0.25f;
  float c, s;
  clk_cossin(3.14159265358979f * (low ? g : 0.5f - g), c, s);
  return low ? s : c;
}

// sample j of the call (-CLK_HIST <= j < cnt), or 0 outside (no output reaches there: the guard only keeps a tile's unused ends inside the buffers)
__device__ __forceinline__ float2 clk_x(const float2 *__restrict__ in, const float2 *__restrict__ hist, long long j, long long cnt)
{
  if (j < -CLK_HIST || j >= cnt) return make_float2(0.f, 0.f);
  return j >= 0 ? in[j] : hist[CLK_HIST + j];
}

// The first cblocks workgroups: lane t of workgroup b computes output m0 + b CLK_THREADS + t of the call's nout outputs into out[b CLK_THREADS + t]; in[0] is
// the stream's sample n0 (absolute), the call has cnt of them.  One workgroup behind them writes the history the next call reads: the last CLK_HIST samples of
// (this call's history, this call's input).  in, out, hist and hist_next do not overlap.
template <int TAPS>
__global__ __launch_bounds__(CLK_THREADS) void clock_kernel(const float2 *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist,
                                                            float2 *__restrict__ hist_next, long long n0, long long cnt, unsigned long long m0, long long nout,
                                                            unsigned cblocks, ClockArgs a)
{
  constexpr int H = TAPS / 2, TILE = clk_tile(TAPS);
  __shared__ float2 tile[TILE];
  if (blockIdx.x >= cblocks) {
    const int k = (int)threadIdx.x;
    if (k < CLK_HIST) hist_next[k] = clk_x(in, hist, cnt - CLK_HIST + k, cnt);      // cnt >= CLK_HIST: all from the input; else the old history moves up by cnt
    return;
  }
  const unsigned long long mb = m0 + (unsigned long long)blockIdx.x * CLK_THREADS;
  const ClockPos pb = clock_pos(a.c, mb);
  const long long j0 = (long long)pb.base - (H - 1) - n0;                             // tile[0]'s index in the call
  for (int i = (int)threadIdx.x; i < TILE; i += CLK_THREADS) tile[i] = clk_x(in, hist, j0 + i, cnt);
  __syncthreads();
  const long long t = (long long)blockIdx.x * CLK_THREADS + threadIdx.x;
  if (t >= nout) return;
  const ClockPos p = clock_pos(a.c, mb + threadIdx.x);
  const int off = (int)(p.base - pb.base);                                            // tile[off + i] = x[base + i - (H - 1)]
  float2 y = tile[off + H - 1];
  if (p.f != 0) {
    const bool up = (p.f >> 63) != 0;
    const unsigned long long g = up ? 0ull - p.f : p.f;
    const float gf = (float)g * 5.421010862427522e-20f;                               // g 2^-64 in (0, 1/2]
    const float d = up ? gf - 1.0f : -gf;                                             // -phi: k - phi = k + d, exact at k = 0 below one half
    const float A = clk_sinpi(gf) * 0.318309886183791f;                               // sin(pi phi) / pi
    float cw, sw;
    clk_cossin((up ? 1.0f - gf : gf) * (3.14159265358979f / (float)(H + 1)), cw, sw);
    const float Ac = A * cw, As = A * sw, Ap = A * 0.54f, An = -Ap;                   // tap k's numerator: -(-1)^k A (0.54 + 0.46 cos(pi (k - phi) / (H + 1)))
    float yr = 0.f, yi = 0.f;
#pragma unroll
    for (int i = 0; i < TAPS; i++) {                                                  // k ascending: the order of the sum is fixed
      const int k = i - (H - 1);
      const float ak = k == 1 ? (up ? gf : 1.0f + d) : (float)k + d;                  // above one half the tap at k = 1 is the near one: 1 - phi = g 2^-64
      const float r = __builtin_amdgcn_rcpf(ak);
      const float h = __builtin_fmaf(a.wc[i], Ac, __builtin_fmaf(a.ws[i], As, (k & 1) ? Ap : An)) * r;
      const float2 x = tile[off + i];
      yr += h * x.x; yi += h * x.y;
    }
    y = make_float2(yr, yi);
  }
  out[t] = y;
}

}  // namespace dvbt
