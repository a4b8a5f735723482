"""The soft decoder's two planners agree: k_soft4.hpp::s4_plan (what a segment launches with) and oracle/o_soft.c::o_soft_plan (what the model is run with).
tests/test_gpu_soft_kernels.py takes the chunk size B and the step count from the test, not from a plan; this is what ties its sizes to what a real segment
would plan.  The host part of the header is compiled for the CPU as it stands (as in tests/test_soft_scratch_bound.py) and linked against the oracle's library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <cstdio>
#include <cstddef>
namespace dvbt {
#include "s4_host.inc"
}
extern "C" void o_soft_plan(long long total_out, int ntb, int *B_out, int *nsteps_out);
using namespace dvbt;
static long long bad = 0, checked = 0;
static int bmin = 1 << 30, bmax = 0;
static void one(long long t, int ntb)
{
  const S4Plan p = s4_plan(t, ntb);
  int B = -1, ns = -1;
  o_soft_plan(t, ntb, &B, &ns);
  checked++;
  if (B != p.B || ns != p.nsteps) { if (bad++ < 5) printf("t %lld ntb %d: s4_plan %d %d, o_soft_plan %d %d\n", t, ntb, p.B, p.nsteps, B, ns); }
  // what the decoder's test hook accepts is what the planner produces
  const int look = 8 * ntb > S4_LOOK ? 8 * ntb : S4_LOOK;
  if (p.B < 64 || p.B > S4_BMAX || p.nsteps % S4_BLK != 0 || p.nsteps > S4_MAXSTEPS || p.nsteps < S4_WARM + 8 * p.B + look || p.nsteps >= S4_WARM + 8 * p.B + look + S4_BLK) bad++;
  if (p.B < bmin) bmin = p.B;
  if (p.B > bmax) bmax = p.B;
}
int main()
{
  const int ntbs[] = {5, 9, 10, 15, 24};
  for (int ni = 0; ni < 5; ni++) {
    for (long long t = 1; t <= 6000000; t += (t < 70000 ? 1 : 97)) one(t, ntbs[ni]);     // the lengths tests/test_soft_scratch_bound.py sweeps
    // the decoder's stream bound for 1, 17 and 65 superframes of 8k QAM64 7/8: calls * payload * m * k / (8 n) + 1, calls = 272 superframes' symbols + the lead-in's
    for (int nsf = 1; nsf <= 65; nsf += (nsf == 1 ? 16 : 48)) {
      const long long calls = (1000 + (long long)nsf * 272 * 8448 + 3 * 8192 - (2 * 8192 + 256 + 16)) / 8448 + 1;
      one(calls * 6048 * 6 * 7 / (8 * 8) + 1, ntbs[ni]);
    }
    for (long long t = 6000000; t <= 400000000; t += 99991) one(t, ntbs[ni]);            // the largest chunk (one round of ~10 M bytes), then several rounds
  }
  printf("%lld violations of %lld, B %d..%d\n", bad, checked, bmin, bmax);
  {   // the headline workload plans a large chunk: 65 superframes
    const long long calls = (1000 + 65ll * 272 * 8448 + 3 * 8192 - (2 * 8192 + 256 + 16)) / 8448 + 1;
    const S4Plan p = s4_plan(calls * 6048 * 6 * 7 / 64 + 1, 24);
    printf("65 superframes: B %d nsteps %d\n", p.B, p.nsteps);
  }
  return bad != 0;
}
"""


def test_the_kernel_header_and_the_model_plan_the_same_chunks(po, tmp_path):
    src = open(os.path.join(ROOT, "gr_dvbt_amd", "csrc", "k_soft4.hpp")).read()
    a, b = src.index("constexpr int S4_WARM"), src.index("struct S4Lane")
    (tmp_path / "s4_host.inc").write_text(src[a:b])
    (tmp_path / "main.cpp").write_text(MAIN)
    exe, odir = str(tmp_path / "s4_plan"), os.path.join(ROOT, "oracle")           # (the po fixture has built oracle/liboracle.so)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", str(tmp_path), "-o", exe, str(tmp_path / "main.cpp"), os.path.join(odir, "liboracle.so"), "-Wl,-rpath," + odir])
    out = subprocess.check_output([exe], text=True)
    lines = out.strip().splitlines()
    assert lines[-2].startswith("0 violations") and lines[-2].endswith("B 64..304"), out
    assert lines[-1] == "65 superframes: B 268 nsteps 2592", out
