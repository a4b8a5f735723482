// k_clock_math.hpp -- the host-callable position arithmetic of k_clock.hpp (the sample-clock offset block, dvbt_clock_*): where output m samples the input,
// as integers, and how many outputs a given number of inputs completes.  The kernel and the host's output count read the same clock_pos.
//
//   P(m) = P0 + m S            in units of 2^-64 input samples: a 128-bit unsigned integer
//   S  = 2^64 + rint(ppm 1e-6 2^64)     (ties to even; 65 bits)            P0 = trunc(start 2^64)
//   base(m) = P(m) >> 64       f(m) = P(m) mod 2^64
#pragma once
#include <cmath>
#include <cstdint>

#ifndef CLOCK_HD
#if defined(__HIPCC__)
#define CLOCK_HD __host__ __device__ __forceinline__
#else
#define CLOCK_HD inline
#endif
#endif

namespace dvbt {

constexpr int CLK_HIST = 64;                 // input samples the handle keeps: taps - 1 <= 63 of them lie in front of a call
constexpr double CLK_MAX_PPM = 1000.0;
constexpr long long CLK_MAX_INDEX = 1ll << 48;   // first_out, first_in
constexpr long long CLK_MAX_TOTAL = 1ll << 56;   // input samples a stream may count: keeps m S inside 128 bits with room to spare

struct ClockStep { unsigned long long s_hi, s_lo, p0_hi, p0_lo; };   // S = s_hi 2^64 + s_lo (s_hi is 0 or 1), P0 = p0_hi 2^64 + p0_lo
struct ClockPos { unsigned long long base, f; };

CLOCK_HD unsigned long long clock_mulhi(unsigned long long a, unsigned long long b)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}

// P(m): the high word of m S is m s_hi + hi(m s_lo), the low word lo(m s_lo); P0's low word carries into the high one
CLOCK_HD ClockPos clock_pos(const ClockStep &c, unsigned long long m)
{
  const unsigned long long lo = m * c.s_lo;
  const unsigned long long hi = (c.s_hi ? m : 0ull) + clock_mulhi(m, c.s_lo);
  ClockPos p;
  p.f = lo + c.p0_lo;
  p.base = hi + c.p0_hi + (p.f < lo ? 1ull : 0ull);
  return p;
}

// The rest is the host's.
// |ppm| <= CLK_MAX_PPM, 0 <= start < 2^31 (the caller has checked).  d = rint(ppm 1e-6 2^64): |d| < 2^55; a negative d is S = 2^64 - |d|, whose low word is d's
// two's complement.  start - floor(start) and its scaling are exact, the conversion truncates.
inline ClockStep clock_step(double ppm, double start)
{
  const long long d = (long long)nearbyint(ldexp(ppm * 1e-6, 64));
  const double whole = floor(start);
  ClockStep c;
  c.s_hi = d >= 0 ? 1ull : 0ull; c.s_lo = (unsigned long long)d;
  c.p0_hi = (unsigned long long)whole; c.p0_lo = (unsigned long long)ldexp(start - whole, 64);
  return c;
}

// E(N): the smallest m >= 0 with base(m) + H >= N -- the outputs in front of it are the ones N input samples complete.  N <= CLK_MAX_INDEX + CLK_MAX_TOTAL.
// The quotient ceil(((N - H) 2^64 - P0) / S) is then set against clock_pos itself, so what is counted is what the kernel computes.
inline unsigned long long clock_E(const ClockStep &c, int H, unsigned long long N)
{
  if (N <= (unsigned long long)H) return 0;
  const unsigned long long need = N - (unsigned long long)H;          // base(m) >= need
  if (c.p0_hi >= need) return 0;
  const unsigned __int128 T = ((unsigned __int128)need << 64) - (((unsigned __int128)c.p0_hi << 64) | c.p0_lo);
  const unsigned __int128 S = ((unsigned __int128)c.s_hi << 64) | c.s_lo;
  unsigned long long m = (unsigned long long)((T + S - 1) / S);
  while (m > 0 && clock_pos(c, m - 1).base >= need) m--;
  while (clock_pos(c, m).base < need) m++;
  return m;
}

}  // namespace dvbt
