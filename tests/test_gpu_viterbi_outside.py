"""What a block of 24 windows does outside its windows (gr_dvbt_amd/csrc/k_viterbi3.hpp: staging's pair table, the per-constellation bit compaction v3_compact, stage_load's
block bounds l_first / l_last with the 16-byte load inside them and the byte-wise path outside) through the single block (dvbt_viterbi_decoder_work), driven as
tests/test_gpu_viterbi_opsel.py drives it: streams of 8 and 40 reference blocks of bsize 48 (48 to 1,680 bytes: one to seven chunk decoders of 264 bytes, so wavefronts with
idle rows), the first chunk's warm-up reaching in front of the stream (its blocks lie in front of l_first wherever the input does not start on a 4-byte boundary of the
lane's loads, and in front of u_first) and the last block past its end (behind l_last: the lanes test their bytes one by one).
 * all five code rates x three constellations: the compaction has one branch per constellation, the pair table's keys depend on the puncture pattern;
 * clean codewords and random symbols: random symbols bring every (four keep flags, four received bits) key of the pair table;
 * the shortcut on and walked (set_viterbi_walk): no differing byte against the oracle's decoder (o_viterbi_decode) and none between the two.
The input's position: the single block copies every call's input behind the history it keeps (at most 8,192 bytes) in a buffer of its own, so the kernel's `in` is that
buffer and what moves is in_base, the stream index of its first byte, and with it the place of every block's first byte in a 4-byte word (stage_load's `off`) and the first
block whose loads all lie inside the input.  test_input_at_every_byte_offset feeds a first call of 8,193 + 3 r bytes (r = 0..3: in_base = 1, 4, 7, 10 in the second call) from
a device pointer that itself stands at byte offset r of its allocation, and a second call behind it.  test_two_calls_on_one_handle: the carried state crosses a call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_viterbi_opsel import _symbols  # noqa: E402
from test_gpu_viterbi_shortcut import _run, g  # noqa: E402,F401
from test_gpu_viterbi_staging import NTB, _oracle, _stream  # noqa: E402

CASES = [(const, cr, kind) for kind in ("clean", "random") for const in range(3) for cr in range(5)]
IDS = [f"c{a}-r{b}-{k}" for a, b, k in CASES]


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
@pytest.mark.parametrize("r", range(4))
def test_input_at_every_byte_offset(po, g, r):  # noqa: F811
    """QAM16 2/3 at bsize 4: 3 input bytes and 1 output byte per reference block.  Call 1: 2,731 + r blocks = 8,193 + 3 r bytes, from a device pointer at byte offset r; the block
    keeps the last 8,192 of them, so call 2 (300 blocks, from a device pointer at offset 3 - r) runs with in_base = 1 + 3 r: 1, 0, 3, 2 mod 4.  One stream, 2 % flipped bits."""
    import torch
    const, cr, bsize = 1, 1, 4
    nb1, nb2 = 2731 + r, 300
    c, d_nsym, d_nout, data, sym = _stream(po, const, cr, bsize, nb1 + nb2, 0.02)
    assert (d_nsym, d_nout) == (3, 1) and (nb1 * d_nsym - 8192) % 4 == (1, 0, 3, 2)[r]
    ref = _oracle(po, c, bsize, sym, (nb1 + nb2) * d_nout)
    b = g.Block("viterbi_decoder", const, 0, cr, bsize, 0, -1)
    s = torch.cuda.Stream()
    outs = []
    for k, (lo, hi, shift) in enumerate(((0, nb1, r), (nb1, nb1 + nb2, 3 - r))):
        x = sym[lo * d_nsym:hi * d_nsym]
        with torch.cuda.stream(s):
            xin = torch.zeros(len(x) + 8, dtype=torch.uint8, device="cuda")
            xin[shift:shift + len(x)] = torch.from_numpy(x.copy()).to("cuda")
            out = torch.zeros((hi - lo) * d_nout + 64, dtype=torch.uint8, device="cuda")
        s.synchronize()
        n, cons, _ = b.work_device((hi - lo) * d_nout, (hi - lo) * d_nsym, xin.data_ptr() + shift, out.data_ptr(), [(0, g.TAG_SUPERFRAME_START, 0xaa)] if k == 0 else [], s.cuda_stream)
        s.synchronize()
        assert cons == len(x)
        outs.append(out[:n].cpu().numpy())
    b.close()
    got = np.concatenate(outs)
    assert len(got) == len(ref) == (nb1 + nb2) * d_nout - NTB[cr]
    assert (got == ref).all(), np.flatnonzero(got != ref)[:5]


@pytest.mark.gpu
def test_two_calls_on_one_handle_give_the_bytes_of_one(po, g):  # noqa: F811
    const, cr = 2, 4
    c, d_nsym, d_nout, sym = _symbols(po, const, cr, 40, "random")
    ref = _oracle(po, c, 48, sym, 40 * d_nout)
    one, _, _ = _run(g, const, cr, sym, d_nsym, d_nout, 0)
    b = g.Block("viterbi_decoder", const, 0, cr, 48, 0, -1)
    outs = []
    for k, (lo, hi) in enumerate(((0, 17), (17, 40))):
        out = np.zeros((hi - lo) * d_nout, np.uint8)
        n, cons, _ = b.work((hi - lo) * d_nout, (hi - lo) * d_nsym, np.ascontiguousarray(sym[lo * d_nsym:hi * d_nsym]), out, [(0, g.TAG_SUPERFRAME_START, 0xaa)] if k == 0 else [])
        assert cons == (hi - lo) * d_nsym
        outs.append(out[:n])
    b.close()
    two = np.concatenate(outs)
    assert len(two) == len(one) == len(ref) == 40 * d_nout - NTB[cr]
    assert (two == one).all(), np.flatnonzero(two != one)[:5]
    assert (one == ref).all(), np.flatnonzero(one != ref)[:5]
