"""One branch-metric permute per trellis step at every phase, as compiled (gr_dvbt_amd/csrc/k_viterbi3.hpp: v3_step; tests/test_viterbi_opsel_model.py holds the argument).
The same compile and the same rule as tests/test_viterbi_isa_renorm.py (tools/vit_window_count.py: 17 v_pk_max_i16 = one trellis window), on viterbi3_kernel<24, 72, 1>, no GPU
needed.

Until round 11 the steps at the phases 1 and 5 issued a second v_perm_b32 for register 1: 32 of the 96 steps of twelve windows, and a block of twelve windows held 130 to 143
v_perm_b32.  Now a block of twelve windows holds
  * one per step (96), one per window for the path-byte word (12) and one per renormalisation (two per twelve windows; three allowed, for the one the compiler moves across its
    block boundary, tests/test_viterbi_isa_renorm.py): at most 96 + 12 + 3;
  * VALU per window: the parent commit's 86.3 (hop-free windows 0-11) / 94.7 (windows 0-11 with hops) / 90.2 (windows 12-23) minus 2.5 -- 32 / 12 = 2.67 instructions per window
    are gone, the remainder is room for instructions that move across the compiler's block boundaries.  As compiled when this test was written: 83.7 / 92.0 / 85.8.  The
    permute alone gives 83.9 / 92.2 / 87.5: the two versions of the windows 0-11 begin alike and the compiler hoists that beginning -- window 0's permutes, three second ones among
    them in the parent -- in front of the branch between them, so their blocks show 29 of the 32.  The rest of the margin comes from the ring's row, masked once per group of
    eight windows (v3_fwd_window) instead of once per window: -3 in the windows 0-11, -20 in the windows 12-23;
  * the kernel's resources: no more VGPRs than the parent's 169 (the twelve second selectors are gone), no scratch, LDS within 80 KB (two workgroups per CU)."""
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
BLOCKS = (("hop-free windows 0-11", 86.3), ("windows 0-11 with hops", 94.7), ("windows 12-23", 90.2))      # the parent commit's VALU per window
SAVED = 2.5


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "dvbt_hip.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(ROOT, "gr_dvbt_amd", "csrc", "dvbt_hip.hip")], stderr=subprocess.DEVNULL)
    return out.read_text()


@pytest.fixture(scope="module")
def blocks(asm):
    b = vit_window_count.windows(asm, KERNEL)
    assert [(n, hops) for _, _, n, hops, _, _ in b] == [(12, False), (12, True), (12, False)]
    return b


def test_one_permute_per_step(blocks):
    for (_, line, n, _, ops, _), (what, _) in zip(blocks, BLOCKS):
        print(f"+{line}: {what}: {ops['v_perm_b32']} v_perm_b32 in {n} windows (at most {96 + 12 + 3})")
        assert ops["v_perm_b32"] <= 96 + 12 + 3, (what, ops["v_perm_b32"])


def test_the_deltas_halves_are_picked_by_op_sel(blocks):
    """the 32 steps at the phases 1 and 5 of twelve windows: an add and a subtract per register, each with its half of the one word on the second source"""
    for (_, _, _, _, _, body), (what, _) in zip(blocks, BLOCKS):
        lo = sum(bool(re.match(r"v_pk_(add_u16|sub_i16) .*op_sel_hi:\[1,0\]", l)) for l in body)
        hi = sum(bool(re.match(r"v_pk_(add_u16|sub_i16) .*op_sel:\[0,1\]", l)) for l in body)
        print(f"{what}: {lo} packed adds/subs on the low half, {hi} on the high half")
        assert lo == 64 and hi == 64, (what, lo, hi)


def test_valu_per_window(blocks):
    for (_, line, n, _, ops, _), (what, parent) in zip(blocks, BLOCKS):
        per = sum(ops.values()) / n
        print(f"+{line}: {what}: {per:.1f} VALU per window (at most {parent} - {SAVED} = {parent - SAVED:.1f})")
        assert per <= parent - SAVED + 1e-9, (what, per)


def test_resources(asm):
    m = re.search(r"\.amdhsa_kernel %s\S*\n(.*?)\.end_amdhsa_kernel" % re.escape(KERNEL), asm, re.S)
    assert m
    f = {a: int(b) for a, b in re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(1))}
    print(f"VGPRs {f['next_free_vgpr']} (at most 169), scratch {f['private_segment_fixed_size']} B, LDS {f['group_segment_fixed_size']} B (at most 81,920)")
    assert f["next_free_vgpr"] <= 169 and f["private_segment_fixed_size"] == 0 and f["group_segment_fixed_size"] <= 81920, f
