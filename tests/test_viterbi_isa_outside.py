"""What viterbi3_kernel<24, 72, 1> issues per block of 24 windows OUTSIDE its windows (gr_dvbt_amd/csrc/k_viterbi3.hpp: staging, the chains' set-up, the shortcut's decision;
DESIGN.md 5, "Outside the windows"), as compiled: the VALU instructions between the steady-state loop's header and the first block of windows, found as
tests/test_viterbi_isa_staging.py finds them (its fixture is used here).  The stretch is a static count -- it holds every path an iteration can take, the three
constellations' compaction branches, the 64-bit locate and the byte-wise loads around the input's ends among them, not the path one iteration takes.
 * 471 at the commit before the pair table, the per-constellation compaction and the loads' block bounds; at least 50 fewer is the condition the change was held to;
 * as compiled with them: 412 (the pair table -30, the compaction's three branches +46 for the one generic sequence, the load inside its bounds and the byte-wise path's
   clamped limits -75); held at that + 4;
 * the steady-path load -- the first global_load_dwordx4 of the stretch, inside the block bounds -- is reached from its label without any 64-bit compare: one aligned
   address, one wave-uniform test of the bounds, one exec mask."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_viterbi_isa_staging import kernel, pytestmark  # noqa: E402,F401

PARENT = 471
AS_COMPILED = 412


def _stretch(kernel):  # noqa: F811
    lines, header, blocks = kernel
    first = min(b[0] for b in blocks if b[0] > header)
    return lines[header:first]


def test_valu_between_the_loop_header_and_the_first_window(kernel):  # noqa: F811
    seg = _stretch(kernel)
    valu = [l.split()[0] for l in seg if l.startswith("v_")]
    wide = sum(bool(re.match(r"v_cmp_\w+_[iu]64", op)) for op in valu)
    print(f"{len(valu)} VALU between the loop header and the first block of windows ({PARENT} before), {wide} of them 64-bit compares")
    assert len(valu) <= PARENT - 50, len(valu)
    assert len(valu) <= AS_COMPILED + 4, len(valu)


def test_steady_path_load_needs_no_64_bit_compare(kernel):  # noqa: F811
    seg = _stretch(kernel)
    loads = [i for i, l in enumerate(seg) if l.startswith("global_load_dwordx4")]
    assert loads and not [l for l in seg if l.startswith("flat_load")], loads       # (a flat load would count as an LDS operation in the waits)
    label = max(i for i in range(loads[0]) if re.match(r"\.?\w+:$", seg[i]))
    path = [l for l in seg[label:loads[0] + 1] if l]
    print("\n".join(path))
    assert not [l for l in path if re.match(r"v_cmp_\w+_[iu]64", l)], path
    assert len([l for l in path if l.startswith("v_")]) <= 12, path                 # (as compiled: 9 -- two compares with the bounds, the address, q zeroed once)
