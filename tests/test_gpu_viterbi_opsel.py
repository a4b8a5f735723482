"""The Viterbi decoder's one branch-metric permute per step (gr_dvbt_amd/csrc/k_viterbi3.hpp: v3_step at the phases 1 and 5, where both registers' deltas come out of one
permuted word through the op_sel of the packed adds) through the single block (dvbt_viterbi_decoder_work), driven as tests/test_gpu_viterbi_renorm.py drives it: streams of 8
and 40 reference blocks of bsize 48, one to seven chunk decoders of 264 bytes, the first chunk's warm-up reaching in front of the stream.
tests/test_viterbi_opsel_model.py holds the argument (every cell receives the delta of its own label class); here the kernel itself decodes
 * all five code rates x three constellations: staging depends on the bits per symbol and on the puncture pattern,
 * clean codewords and random symbols: the deltas of the phases 1 and 5 depend on every received pair, and random symbols bring every (keep flags, received pair) there.
Every case allows no differing byte against the oracle's decoder (o_viterbi_decode) and none against the same input with the traceback's shortcut switched off
(set_viterbi_walk(1)): both versions of a block's first twelve windows run.  The 40-block stream fed in two work() calls on one handle -- the carried state crosses a call --
gives the bytes of the single call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_viterbi_shortcut import _run, _stream, g  # noqa: E402,F401
from test_gpu_viterbi_staging import NTB, _oracle  # noqa: E402

CASES = [(const, cr, kind) for kind in ("clean", "random") for const in range(3) for cr in range(5)]
IDS = [f"c{a}-r{b}-{k}" for a, b, k in CASES]


def _symbols(po, const, cr, nblocks, kind):
    c, d_nsym, d_nout, sym = _stream(po, const, cr, nblocks, 0.0)
    if kind == "random":
        sym = np.random.RandomState(5200 + 7 * const + cr).randint(0, 1 << c.m, len(sym)).astype(np.uint8)
    return c, d_nsym, d_nout, sym


@pytest.mark.gpu
@pytest.mark.parametrize("const,cr,kind", CASES, ids=IDS)
@pytest.mark.parametrize("nblocks", [8, 40])
def test_bytes_are_the_oracles_and_the_walked_ones(po, g, const, cr, kind, nblocks):  # noqa: F811
    c, d_nsym, d_nout, sym = _symbols(po, const, cr, nblocks, kind)
    ref = _oracle(po, c, 48, sym, nblocks * d_nout)
    got, short, walked = _run(g, const, cr, sym, d_nsym, d_nout, 0)
    got_w, short_w, walked_w = _run(g, const, cr, sym, d_nsym, d_nout, 1)
    print(f"const {const} rate {cr} {kind} {nblocks} blocks, {len(ref)} bytes: shortcut {short}, walked {walked}")
    assert len(got) == len(got_w) == len(ref) == nblocks * d_nout - NTB[cr]
    assert (got == ref).all(), np.flatnonzero(got != ref)[:5]
    assert (got_w == ref).all(), np.flatnonzero(got_w != ref)[:5]
    assert (got == got_w).all()
    assert short_w == 0 and walked_w == short + walked


@pytest.mark.gpu
def test_two_calls_on_one_handle_give_the_bytes_of_one(po, g):  # noqa: F811
    const, cr = 1, 2
    c, d_nsym, d_nout, sym = _symbols(po, const, cr, 40, "random")
    ref = _oracle(po, c, 48, sym, 40 * d_nout)
    one, _, _ = _run(g, const, cr, sym, d_nsym, d_nout, 0)
    b = g.Block("viterbi_decoder", const, 0, cr, 48, 0, -1)
    outs = []
    for k, (lo, hi) in enumerate(((0, 20), (20, 40))):
        out = np.zeros((hi - lo) * d_nout, np.uint8)
        r, cons, _ = b.work((hi - lo) * d_nout, (hi - lo) * d_nsym, np.ascontiguousarray(sym[lo * d_nsym:hi * d_nsym]), out, [(0, g.TAG_SUPERFRAME_START, 0xaa)] if k == 0 else [])
        assert cons == (hi - lo) * d_nsym
        outs.append(out[:r])
    b.close()
    two = np.concatenate(outs)
    assert len(two) == len(one) == len(ref) == 40 * d_nout - NTB[cr]
    assert (two == one).all(), np.flatnonzero(two != one)[:5]
    assert (one == ref).all(), np.flatnonzero(one != ref)[:5]
