"""The traceback's shortcut over chained best states (gr_dvbt_amd/csrc/k_viterbi3.hpp: link_reads / links_hold and the decision in v3_decode's loop) through the single block
(dvbt_viterbi_decoder_work), as tests/test_gpu_viterbi_staging.py drives it: streams of 8 and 40 reference blocks of bsize 48 (48 to 1,680 bytes: one to seven chunk decoders
of 264 bytes), QPSK and 64-QAM at all five rates.  Every case allows no differing byte against the oracle's decoder (o_viterbi_decode) and none against the same input decoded
with the shortcut switched off (set_viterbi_walk(1)), and looks at the two counters (blocks of 24 windows, per wavefront: bytes by the shortcut / chains walked).

Where the blocks lie: a chunk decoder's relative window r is the stream's window b0 + r - 70, chunks are 264 = 11 x 24 bytes, so every decoder's blocks start at the stream's
windows 2 + 24 k; window w decodes the trellis steps 8 (w - 1) - 2 .. 8 (w - 1) + 5.

What the counters may be, by reasoning (tests/test_viterbi_shortcut_model.py prints the model's shares):
 * clean codeword: the best states chain up everywhere behind a decoder's cold start, which lies inside the warm-up (no call ends there).  A wavefront can walk only where a block
   of one of its decoders holds windows outside the stream, and in the iteration behind it (the decision asks for the block before too): the stream's first chunk (its warm-up
   lies before the stream, up to relative window 70: the iterations of the blocks at 72, one call, and perhaps 96) and the block cut by the stream's end with the one behind it,
   where a longer decoder of the same wavefront still delivers -- at most 4 per wavefront and launch;
 * every case: the model decoder of tests/test_viterbi_shortcut_model.py runs over the same received symbols (_predict): shortcut + walked is the number of iterations in which a
   chain ends in a call, the shortcut counter is at most, and the walked one at least, what the model's links allow;
 * 2 % flipped bits: the model has at most 5 of 24 blocks on the shortcut with ONE decoder per wavefront (rate 1/2; none at the other rates), fewer with four: the
   shortcut counter is 0 at the rates 2/3 to 7/8 and at most a fifth of the iterations at rate 1/2."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rxref  # noqa: E402
import test_viterbi_shortcut_model as model  # noqa: E402
from test_gpu_viterbi_staging import K_OF_RATE, N_OF_RATE, M_OF_CONST, NTB, _oracle  # noqa: E402

CONFIGS = [(const, cr) for const in (0, 2) for cr in range(5)]
IDS = [f"c{a}-r{b}" for a, b in CONFIGS]
CHUNK = 264                                                          # bytes per chunk decoder of the single block (dvbt_blocks.inc)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    return gr_dvbt_amd


def _stream(po, const, cr, nblocks, ber, seed=0):
    c = po.cfg(const, cr, po.T2k)
    d_nsym, d_nout = 48 * c.n // c.m, 48 * c.k // 8
    data, sym = rxref.coded_symbols(po, c, d_nout * nblocks + 64, ber, 1700 + 7 * const + cr + seed)
    return c, d_nsym, d_nout, np.ascontiguousarray(sym[:d_nsym * nblocks])


def _flip(sym, c, step, nbits):
    """flip nbits consecutive received bits, the first of them the first one at or behind trellis step `step` (n received bits per k steps)"""
    p = -(-step * c.n // c.k)
    for q in range(p, p + nbits):
        sym[q // c.m] ^= 1 << (c.m - 1 - q % c.m)


def _model_links(sym, c, cr):
    """(link[w], windows that lie inside the stream) of the reference decoder (tests/test_viterbi_shortcut_model.py) over the received symbols, the windows numbered as the
    kernel numbers them: window w decodes the steps 8 w - 10 .. 8 w - 3, so ten erased steps stand in front"""
    bits = np.unpackbits(sym[:, None], axis=1)[:, 8 - c.m:].reshape(-1).astype(np.int64)
    steps = len(bits) * c.k // c.n
    keep = np.resize(np.array(model.PUNCT[cr], np.int64), 2 * steps)
    rx = np.zeros(2 * steps, np.int64)
    rx[keep == 1] = bits[:int(keep.sum())]
    pad = np.zeros((10, 2), np.int64)
    tab, best = model._decode(np.concatenate([pad, rx.reshape(-1, 2)]), np.concatenate([pad, keep.reshape(-1, 2)]))
    link = np.zeros(len(best), bool)
    link[1:] = (tab[np.arange(1, len(best)), best[1:]] >> 2) == best[:-1]
    return link, len(best)


def _predict(sym, c, cr):
    """What the model says about the launch's counters: (iterations in which a chain ends in a call = shortcut + walked, the most that can be on the shortcut, the fewest that
    must walk).  The kernel's loop per wavefront (k_viterbi3.hpp): iteration jp = 0, 24, .. looks at the block of windows jp .. jp + 23 of each of its up to four decoders (chunk d:
    the stream's windows 264 d - 70 + jp ..) that still has a call to deliver, and takes the shortcut when every link of that block and of the block before holds.  A decoder is the
    streaming decoder -- the model -- from its chunk's first window on (relative window 72: the launch's proof); a block that reaches into the warm-up or past the stream's end is
    `unknown`: it counts as holding for the upper bound and as nothing for the lower one."""
    link, nreal = _model_links(sym, c, cr)
    ntb = NTB[cr]
    total_out = len(sym) * c.m * c.k // c.n // 8 - ntb
    nch = -(-total_out // CHUNK)
    first = 71 + ntb                                                 # relative window of the chain that delivers a chunk's first byte
    J = -(-(72 + CHUNK + ntb - 1) // 24) * 24
    n_ends = short_max = walked_min = 0
    for wave in range(-(-nch // 4)):
        decs = [(CHUNK * d, min(CHUNK, total_out - CHUNK * d)) for d in range(4 * wave, min(4 * wave + 4, nch))]
        for jp in range(0, J - 24, 24):
            ends = any(0 <= jj - first < n for _, n in decs for jj in range(jp, jp + 24))
            known_bad = unknown_or_ok = False
            all_ok = True
            for b0, n in decs:
                if not jp - first < n:
                    continue                                         # (no call left: its links are nobody's)
                for blk in (jp, jp - 24):
                    a0 = b0 - 70 + blk
                    if blk < 72 or a0 + 24 > nreal:
                        continue                                     # unknown
                    if not link[a0:a0 + 24].all():
                        known_bad, all_ok = True, False
            n_ends += ends
            short_max += ends and all_ok
            walked_min += ends and known_bad
    return n_ends, short_max, walked_min


def _run(g, const, cr, sym, d_nsym, d_nout, walk):
    """one call on a fresh handle: (bytes, shortcut iterations, walked iterations)"""
    b = g.Block("viterbi_decoder", const, 0, cr, 48, 0, -1)
    b.set_viterbi_walk(walk)
    nb = len(sym) // d_nsym
    out = np.zeros(nb * d_nout, np.uint8)
    r, cons, _ = b.work(nb * d_nout, nb * d_nsym, sym, out, [(0, g.TAG_SUPERFRAME_START, 0xaa)])
    assert cons == len(sym)
    short, walked = b.viterbi_shortcut()
    b.close()
    return out[:r], short, walked


def _check(po, g, const, cr, c, sym, d_nsym, d_nout):
    nb = len(sym) // d_nsym
    ref = _oracle(po, c, 48, sym, nb * d_nout)
    got, short, walked = _run(g, const, cr, sym, d_nsym, d_nout, 0)
    got_w, short_w, walked_w = _run(g, const, cr, sym, d_nsym, d_nout, 1)
    assert len(got) == len(got_w) == len(ref) == nb * d_nout - NTB[cr]
    assert (got == ref).all(), np.flatnonzero(got != ref)[:5]
    assert (got_w == ref).all(), np.flatnonzero(got_w != ref)[:5]
    assert short_w == 0 and walked_w == short + walked, (short_w, walked_w, short, walked)     # switched off: the same iterations, all walked
    waves = -(-(-(-len(ref) // CHUNK)) // 4)
    n_ends, short_max, walked_min = _predict(sym, c, cr)
    print(f"const {const} rate {cr} {nb} blocks, {len(ref)} bytes, {waves} wavefronts: shortcut {short}, walked {walked}; the model: {n_ends} iterations with calls, "
          f"at most {short_max} on the shortcut, at least {walked_min} walked")
    assert short + walked == n_ends and short <= short_max and walked >= walked_min, (short, walked, n_ends, short_max, walked_min)
    return short, walked, waves


@pytest.mark.gpu
@pytest.mark.parametrize("const,cr", CONFIGS, ids=IDS)
@pytest.mark.parametrize("nblocks", [8, 40])
def test_clean_codeword(po, g, const, cr, nblocks):
    c, d_nsym, d_nout, sym = _stream(po, const, cr, nblocks, 0.0)
    short, walked, waves = _check(po, g, const, cr, c, sym, d_nsym, d_nout)
    assert short > 0 and walked <= 4 * waves, (short, walked, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("const,cr", CONFIGS, ids=IDS)
@pytest.mark.parametrize("pairs", [0, 1], ids=["single", "pairs"])
def test_isolated_flips_around_block_boundaries(po, g, const, cr, pairs):
    """flips in the first window of a block (block 1: window 26), the last window of a block (block 2: window 73), the window in front of a block boundary (window 97), two
    adjacent blocks (4 and 5: windows 110 and 134), then four clean blocks (6 to 9) -- single bits, or pairs of neighbouring bits (with a single one among them), each in the
    LAST step of its window: there a flipped bit leaves the path that differs in the newest input level with (rate 1/2: one bit) or ahead of (two bits) the transmitted one, so the
    window's best state moves and the link of the window behind it fails -- in the model at two to five of the five places for single bits and at all five for pairs; a flip in the
    middle of a window is corrected before the window ends and breaks nothing at rates 1/2 and 2/3.  The bytes are the oracle's and the walked ones; the model must see more
    walked iterations than on the same stream without the flips, the decoder walks more than it does on that stream, and the clean stretch is on the shortcut: shortcut ->
    walk -> shortcut and the previous block's verdict are exercised."""
    c, d_nsym, d_nout, sym = _stream(po, const, cr, 40, 0.0, seed=pairs)
    _, _, walked_min_clean = _predict(sym, c, cr)
    _, _, walked_clean = _run(g, const, cr, sym, d_nsym, d_nout, 0)
    for w, n in ((26, 1 + pairs), (73, 1 + pairs), (97, 1), (110, 1 + pairs), (134, 1 + pairs)):
        _flip(sym, c, 8 * w - 3, n)
    assert _predict(sym, c, cr)[2] > walked_min_clean
    short, walked, waves = _check(po, g, const, cr, c, sym, d_nsym, d_nout)
    assert short > 0 and walked > walked_clean, (short, walked, walked_clean)


@pytest.mark.gpu
@pytest.mark.parametrize("const,cr", CONFIGS, ids=IDS)
def test_two_percent_flipped_bits(po, g, const, cr):
    """the shortcut counter stays near 0: no more than the model allows on the same stream (_check), and that is nothing at the rates 2/3 to 7/8 and at most a fifth of the
    iterations at rate 1/2"""
    c, d_nsym, d_nout, sym = _stream(po, const, cr, 40, 0.02)
    n_ends, short_max, _ = _predict(sym, c, cr)
    assert short_max == 0 if cr >= 1 else 5 * short_max <= n_ends, (n_ends, short_max)
    short, walked, waves = _check(po, g, const, cr, c, sym, d_nsym, d_nout)
    assert short <= short_max, (short, short_max)


@pytest.mark.gpu
def test_segment_api_2k_qam16_1_2_proof_and_repair(po, g):
    """three superframes of 2k QAM16 1/2 through the segment API: the default proof (MODE 1 decoders) and viterbi_verify = 4 (the hand-over to the MODE 2 decoders, which
    share v3_decode and its shortcut, for every chunk the warm-up does not prove -- tests/test_gpu_warmup.py holds that path on a noisy stream) deliver the oracle's TS;
    the switch changes nothing"""
    c = po.cfg(1, 0, po.T2k)
    ibits = c.payload * c.m * c.k // c.n
    iq = po.tx(c, po.make_ts((272 * ibits * 3) // (204 * 8), 23), lead_in=600, tail=3 * c.N)
    o = po.rx(c, iq, want=("ts",))
    ref = np.asarray(o["ts"]).reshape(-1)
    assert ref.size > 0
    for kw in (dict(), dict(viterbi_verify=4)):
        for walk in (0, 1):
            rx = g.Rx(1, 0, po.T2k, max_samples=len(iq), taps=True, **kw)
            rx.set_viterbi_walk(walk)
            rx.run(iq)
            ts = np.asarray(rx.tap(g.TAP_TS)).reshape(-1)
            short, walked = rx.viterbi_shortcut()
            rx.close()
            print(f"{kw} walk {walk}: shortcut {short}, walked {walked}")
            assert ts.size == ref.size and (ts == ref).all(), (kw, walk, np.flatnonzero(ts != ref)[:5])
            assert (short == 0) == bool(walk) and walked > 0
