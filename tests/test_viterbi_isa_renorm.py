"""The renormalisation cadence of the Viterbi decoder as compiled (gr_dvbt_amd/csrc/k_viterbi3.hpp: V3_RENORM_EVERY, v3_window_end).  The same compile and the same rule as
tests/test_viterbi_isa_budget.py (tools/vit_window_count.py: 17 v_pk_max_i16 = one trellis window), on viterbi3_kernel<24, 72, 1>, no GPU needed.

A renormalisation is five VALU instructions: v_and + v_add (the offset at the metric position), one v_perm_b32 that copies it into both halves -- the only v_perm_b32 of the
kernel whose two sources are the same register -- and two v_pk_sub_i16.  With one every second window a block of twelve windows held six of them (5 and 7 as compiled, where
the compiler moved one across a block boundary) and cost 88.0 VALU per window (hop-free windows 0-11), 96.3 (windows 0-11 with traceback hops) and 91.8 (windows 12-23).  One
every six windows takes 8 x 5 instructions out of 24 windows: 1.67 per window.  The bounds are those figures minus 1.67 plus 0.3, the amount by which instructions move across the
compiler's block boundaries from build to build:
  * hop-free windows 0-11: at most 86.7 VALU per window (as compiled when this test was written: 86.3);
  * windows 0-11 with hops: at most 95.0 (94.7);
  * windows 12-23: at most 90.5 (90.2);
  * every block of twelve windows holds exactly two renormalisations."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vit_window_count  # noqa: E402
from gr_dvbt_amd import binding  # noqa: E402

HIPCC = binding.hipcc() if os.path.exists(binding.hipcc()) else shutil.which("hipcc")     # (the compiler that builds the library: without it there is nothing to test)
KERNEL = "_ZN4dvbt15viterbi3_kernelILi24ELi72ELi1E"
SAME_SOURCES = re.compile(r"v_perm_b32\s+v\d+,\s*(v\d+),\s*\1,")


@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "dvbt_hip.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(ROOT, "gr_dvbt_amd", "csrc", "dvbt_hip.hip")], stderr=subprocess.DEVNULL)
    return vit_window_count.windows(out.read_text(), KERNEL)


def test_the_kernel_is_three_blocks_of_twelve_windows(blocks):
    """in program order: the hop-free windows 0-11, the windows 0-11 with hops, the windows 12-23"""
    assert [(n, hops) for _, _, n, hops, _, _ in blocks] == [(12, False), (12, True), (12, False)]


def test_windows_per_block_budget(blocks):
    for (_, line, n, hops, ops, _), (what, bound) in zip(blocks, (("hop-free windows 0-11", 86.7), ("windows 0-11 with hops", 95.0), ("windows 12-23", 90.5))):
        per = sum(ops.values()) / n
        print(f"+{line}: {what}: {per:.1f} VALU per window (at most {bound})")
        assert per <= bound, (what, per)


def test_two_renormalisations_per_twelve_windows(blocks):
    """Counted per basic block, with the one move the compiler makes: both versions of the windows 0-11 end in the same instructions -- the renormalisation of window 11 -- and
    the compiler merges that tail into the block they both continue in, the windows 12-23 (with one renormalisation every second window it left 5, 5 and 7 of the 6 per block in
    the same way).  So a version of the windows 0-11 shows its two or, with window 11's merged away, one; the windows 12-23 show what is missing, the same for both versions;
    and either way through the 24 windows there are exactly four."""
    n_free, n_hops, n_second = (sum(bool(SAME_SOURCES.match(l)) for l in body) for _, _, _, _, _, body in blocks)
    print(f"renormalisations: {n_free} in the hop-free windows 0-11, {n_hops} in the windows 0-11 with hops, {n_second} in the windows 12-23")
    assert n_free == n_hops and n_free in (1, 2), (n_free, n_hops)
    assert n_free + n_second == 4 and n_hops + n_second == 4, (n_free, n_hops, n_second)
