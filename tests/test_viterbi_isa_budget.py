"""The Viterbi decoder's time goes to VALU issue, and how many instructions it issues is a property of what the compiler makes of
gr_dvbt_amd/csrc/k_viterbi3.hpp.  This test compiles the library's device code to gfx950 assembly (no GPU needed) and holds the dominant kernel, viterbi3_kernel<24, 72, 1>,
to its budget with tools/vit_window_count.py's rule (17 v_pk_max_i16 = one trellis window):
  * a block of windows with traceback hops: at most 101.0 VALU per window (the design: 90.5 + 2 per chain and hop);
  * any other block of windows: at most 92.2;
  * no v_add3_u32 and no v_and_b32 with the old ring mask 0x3fc0 in hop windows (a hop is one decrement and one v_bfi_b32: no base address, no separate masks);
  (as compiled when this test was written: 95.7 with hops, 91.5 and 87.9 without; the parent commit: 106.8, 92.2 and 94.0 in a loop of six)
  * LDS per workgroup <= 81,920 B (two per CU beside the symbol kernel's 76 KB), <= 256 VGPRs, no scratch -- for all four kernels that share v3_decode."""
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

HIPCC = binding.hipcc() if os.path.exists(binding.hipcc()) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc not installed")
KERNEL = "_ZN4dvbt15viterbi3_kernelILi24ELi72ELi1E"
SHARED = ("viterbi3_kernelILi24ELi72ELi1E", "viterbi_repair_kernelILi24E", "viterbi_repair_seq_kernelILi24E", "viterbi_fix_kernelILi24E")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "dvbt_hip.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(ROOT, "gr_dvbt_amd", "csrc", "dvbt_hip.hip")], stderr=subprocess.DEVNULL)
    return out.read_text()


def test_window_budget(asm):
    blocks = vit_window_count.windows(asm, KERNEL)
    assert sum(n for _, _, n, hops, _, _ in blocks if hops) == 12 and sum(n for _, _, n, hops, _, _ in blocks if not hops) >= 24, [(n, h) for _, _, n, h, _, _ in blocks]
    for _, line, n, hops, ops, body in blocks:
        per = sum(ops.values()) / n
        print(f"+{line}: {n} windows{' with hops' if hops else ''}: {per:.1f} VALU per window")
        assert per <= (101.0 if hops else 92.2), (line, n, hops, per)
        if hops:
            assert ops["v_bfi_b32"] == 2 * 23, ops["v_bfi_b32"]          # ntraceback - 1 = 23 hops of two chains
            assert not ops["v_add3_u32"]
            assert not [l for l in body if l.startswith("v_and_b32") and "0x3fc0" in l]


def test_resource_limits(asm):
    for k in SHARED:
        m = re.search(r"\.amdhsa_kernel _ZN4dvbt\d+%s\S*\n(.*?)\.end_amdhsa_kernel" % k, asm, re.S)
        assert m, k
        f = {a: int(b) for a, b in re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(1))}
        print(k, f["group_segment_fixed_size"], f["next_free_vgpr"], f["private_segment_fixed_size"])
        assert f["group_segment_fixed_size"] <= 81920 and f["next_free_vgpr"] <= 256 and f["private_segment_fixed_size"] == 0, (k, f)
