"""How viterbi3_kernel<24, 72, 1> stages a block of 24 windows and ends its traceback chains is a property of the order in which the compiler leaves the LDS
operations of gr_dvbt_amd/csrc/k_viterbi3.hpp ("Staging and the traceback's ends"): a wavefront that waits out an LDS round trip leaves the SIMD's
issue port to the one other wavefront.  This test compiles the library's device code to gfx950 assembly (no GPU needed) and holds, in the steady-state loop body:
  * between the loop header and the first block of windows at most 3 `s_waitcnt lgkmcnt(0)`: the compacted bits, the batch of twelve table look-ups, the first
    window's step words (as compiled when this test was written: 2; the parent commit: 15 -- every look-up was waited for and stored before the next was issued,
    and the two best-state reads of the chains' start were waited for on the spot);
  * the step words leave with ds_write_b128 and at most 3 LDS stores (the parent: twelve ds_write_b32);
  * behind the last hop (the last v_bfi_b32 of the block with hops) no ds_read_u8 is waited for on the spot, up to the next block of windows (the parent: both
    chains' last path byte, one after the other, each under its own exec mask behind an s_cbranch_execz: ds_read_u8, s_waitcnt lgkmcnt(0), 12 instructions,
    global_store_byte).
The blocks of windows are found with tools/vit_window_count.py's rule (17 v_pk_max_i16 = one window), as in tests/test_viterbi_isa_budget.py."""
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


def _strip(line):
    return re.sub(r"\s*;.*$", "", line.strip())


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    """the kernel's lines (comments stripped; labels and empty lines kept so that indices are vit_window_count's), the index of the loop header, the blocks of windows"""
    out = tmp_path_factory.mktemp("isa") / "dvbt_hip.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(ROOT, "gr_dvbt_amd", "csrc", "dvbt_hip.hip")], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    m = re.findall(r"^(%s\S*):[^\n]*\n(.*?)\.Lfunc_end" % re.escape(KERNEL), asm, re.S | re.M)
    assert len(m) == 1
    raw = m[0][1].split("\n")
    headers = [i for i, l in enumerate(raw) if "Loop Header" in l]
    blocks = [(start, n, hops, len(body)) for _, start, n, hops, _, body in vit_window_count.windows(asm, KERNEL)]
    # the steady-state loop: the one whose header is followed by the block of windows with hops
    hop = [b for b in blocks if b[2]]
    assert len(hop) == 1
    header = max(h for h in headers if h < hop[0][0])
    return [_strip(l) for l in raw], header, blocks


def _block_end(lines, start):
    """index of the branch or label that ends the basic block starting at `start`"""
    i = start
    while not (lines[i].startswith(("s_cbranch", "s_branch", "s_endpgm")) or (re.match(r"\.?\w+:$", lines[i]) and i > start)):
        i += 1
    return i


def test_staging_waits_and_wide_stores(kernel):
    lines, header, blocks = kernel
    first = min(b[0] for b in blocks if b[0] > header)
    seg = lines[header:first]
    waits = sum(l == "s_waitcnt lgkmcnt(0)" for l in seg)
    stores = [l.split()[0] for l in seg if l.startswith("ds_write")]
    print(f"loop header +{header}, first block of windows +{first}: {waits} x lgkmcnt(0), LDS stores {stores}")
    assert waits <= 3, waits
    # the compacted bits take one store per constellation (one, two or three words: three exclusive branches), the step words three
    wide = [s for s in stores if s == "ds_write_b128"]
    assert len(wide) == 3, stores
    narrow_after_lut = stores[stores.index("ds_write_b128"):]
    assert narrow_after_lut == ["ds_write_b128"] * 3, stores         # nothing but the three wide stores from the first of them on


def test_chain_ends_are_not_waited_for_on_the_spot(kernel):
    lines, header, blocks = kernel
    hop = [b for b in blocks if b[2]][0]
    end = _block_end(lines, hop[0])
    last_bfi = max(i for i in range(hop[0], end) if lines[i].startswith("v_bfi_b32"))
    nxt = min((b[0] for b in blocks if b[0] > end), default=len(lines))
    def code(a, b):
        return [l for l in lines[a:b] if l and not re.match(r"\.?\w+:$", l)]
    # both chains' last path byte are read inside the block with hops, together: nothing but the other read between them
    inside = code(last_bfi, end)
    reads = [i for i, l in enumerate(inside) if l.startswith("ds_read_u8")]
    print(f"last v_bfi_b32 +{last_bfi}, block ends +{end}: {len(reads)} ds_read_u8 behind it, inside the block")
    assert len(reads) == 2 and reads[1] == reads[0] + 1, inside[:8]
    # no path byte is waited for on the spot, up to the next block of windows (the branch target may lie in front of the header: the stretch that follows in the file is looked at too)
    stretch = code(last_bfi, min(nxt, end + 200))
    for i, l in enumerate(stretch[:-1]):
        if l.startswith("ds_read_u8"):
            assert stretch[i + 1] != "s_waitcnt lgkmcnt(0)", stretch[i:i + 3]
    assert not [l for l in lines[last_bfi:end] if l.startswith("s_cbranch")]
