"""v3_compact<M> (gr_dvbt_amd/csrc/k_viterbi3.hpp), the per-constellation bit compaction of staging: the function's source is cut out of the header and compiled for the
host (as tests/test_rs_lane_host.py does with the RS lane decoder), then compared with the literal formula it replaces,
    grp(d) = ((d & mk) << 3 m) | (((d >> 8) & mk) << 2 m) | (((d >> 16) & mk) << m) | ((d >> 24) & mk),   mk = (1 << m) - 1,
on 10^5 random dwords for m = 2, 4, 6 -- all 32 bits random, so the bits above a byte's m valid ones hold garbage -- and on the words of all ones, all zeros and single bits."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <cstdio>
#include <cstdint>
#define __device__
#define __forceinline__ inline
#include "compact_fn.inc"
static unsigned grp(unsigned d, int m)
{
  const unsigned mk = (1u << m) - 1;
  return ((d & mk) << (3 * m)) | (((d >> 8) & mk) << (2 * m)) | (((d >> 16) & mk) << m) | ((d >> 24) & mk);
}
int main()
{
  uint64_t s = 0x9e3779b97f4a7c15ull;
  long bad = 0, total = 0;
  for (int i = 0; i < 100000 + 34; i++) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;                        // xorshift64
    unsigned d = (unsigned)(s >> 16);
    if (i >= 100000) { const int j = i - 100000; d = j == 0 ? 0u : j == 1 ? ~0u : 1u << (j - 2); }
    const unsigned got[3] = {v3_compact<2>(d), v3_compact<4>(d), v3_compact<6>(d)};
    for (int k = 0; k < 3; k++) {
      total++;
      if (got[k] != grp(d, 2 * k + 2)) { if (bad < 10) printf("MISMATCH m %d d %08x: %08x, formula %08x\n", 2 * k + 2, d, got[k], grp(d, 2 * k + 2)); bad++; }
    }
  }
  printf("%ld mismatches of %ld\n", bad, total);
  return bad != 0;
}
"""


def test_compaction_equals_the_formula(tmp_path):
    src = open(os.path.join(ROOT, "gr_dvbt_amd", "csrc", "k_viterbi3.hpp")).read()
    a, b = src.index("template <int M> __device__ __forceinline__ unsigned v3_compact"), src.index("// (end of v3_compact)")
    (tmp_path / "compact_fn.inc").write_text(src[a:b])
    (tmp_path / "compact_host.cpp").write_text(MAIN)
    exe = str(tmp_path / "compact_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", str(tmp_path), "-o", exe, str(tmp_path / "compact_host.cpp")])
    out = subprocess.check_output([exe], text=True)
    assert out.strip().endswith("0 mismatches of 300102"), out
