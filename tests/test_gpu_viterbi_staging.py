"""The Viterbi decoder alone (dvbt_viterbi_decoder_work / _work_device) at the stream lengths where the staging of a block of windows can go wrong
(gr_dvbt_amd/csrc/k_viterbi3.hpp, stage_words / trace_init / v3_trace_store): a decoder whose warm-up reaches before the stream's start, blocks cut by
the stream's end (the u_first / u_last clamp), a last chunk shorter than one block of 24 windows, chunks of one and two blocks through the segment API.
Every case compares with the oracle's decoder (o_viterbi_decode, or the oracle receiver's Viterbi tap) and allows no differing byte; the channel
flips 1 to 2 % of the coded bits, so best states and tracebacks matter.

Stream lengths.  A block of windows is 192 trellis steps = 24 output bytes, a lane stages 12 of the steps.  Every legal stream is a whole number of
bytes (viterbi_decoder_impl.cc requires k * bsize to be a multiple of 8), so the stream's end can stand at 24 places of a block -- a residue of the
step count mod 192 that is not a multiple of 8 (1, 11, 13, 191) cannot be fed to the block.  At bsize 48 alone the step count 48 k n mod 192 takes
four values; the sweep therefore runs twice: 1 to 40 reference blocks of bsize 48 for every constellation and rate, and 24 consecutive lengths at each
configuration's smallest legal bsize, which at rates 2/3, 5/6 (and 1/2, 7/8 below 64-QAM) moves the end byte by byte through all 24 places: windows 0, 1,
11, 12, 13 and 23 of a block (steps 0, 8, 88, 96, 104, 184 mod 192) among them, every third of a block, asserted below.  One consequence: a block's step 0
is real step 8 w - 10 of the stream, so the stream's last real step falls on 3 of a lane's 12 staged positions (a lane's first step is 8 w - 10 + 12 pl, so stage_words' `hi` is 2, 6 or 10 in
the lane that holds it), not on each of the twelve; the other nine cannot be produced through the block or the segment API."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rxref  # noqa: E402

K_OF_RATE, N_OF_RATE, M_OF_CONST = (1, 2, 3, 5, 7), (2, 3, 4, 6, 8), (2, 4, 6)
NTB = (5, 9, 10, 15, 24)
CONFIGS = [(const, cr) for const in range(3) for cr in range(5)]
IDS = [f"c{a}-r{b}" for a, b in CONFIGS]


def _legal(bsize, const, cr):
    k, n, m = K_OF_RATE[cr], N_OF_RATE[cr], M_OF_CONST[const]
    return (2 * k * bsize) % 16 == 0 and (bsize * n) % m == 0 and (bsize * k) % 8 == 0


def _small_bsize(const, cr):
    return next(b for b in range(1, 49) if _legal(b, const, cr))


def _ber(const, cr):
    return 0.01 + 0.0025 * ((const + 2 * cr) % 5)                  # 0.01 .. 0.02


def _small_lengths(const, cr):
    """24 consecutive stream lengths in reference blocks, from the first that is longer than one chunk decoder's warm-up-free start (30 bytes + ntraceback)"""
    d_nout = _small_bsize(const, cr) * K_OF_RATE[cr] // 8
    first = -(-(30 + NTB[cr]) // d_nout)
    return range(first, first + 24)


def _steps(bsize, cr, nblocks):
    return K_OF_RATE[cr] * bsize * nblocks


def test_the_sweeps_reach_every_place_of_a_block():
    """(no GPU) the residues of the total step count mod 192 that the two sweeps feed: at least 16, with the first, second, the two around the middle and
    the last window of a block, for every constellation"""
    for const in range(3):
        res = set()
        for cr in range(5):
            res |= {_steps(48, cr, nb) % 192 for nb in range(1, 41)}
            res |= {_steps(_small_bsize(const, cr), cr, nb) % 192 for nb in _small_lengths(const, cr)}
        assert len(res) >= 16 and {0, 8, 88, 96, 104, 184} <= res, (const, sorted(res))
        assert all(any(lo <= r < lo + 64 for r in res) for lo in (0, 64, 128))
        assert res == {8 * w for w in range(24)}


def _stream(po, const, cr, bsize, nblocks, ber):
    c = po.cfg(const, cr, po.T2k)
    d_nsym, d_nout = bsize * c.n // c.m, bsize * c.k // 8
    data, sym = rxref.coded_symbols(po, c, d_nout * nblocks + 64, ber, 900 + 7 * const + cr + bsize)
    return c, d_nsym, d_nout, data, np.ascontiguousarray(sym[:d_nsym * nblocks])


def _oracle(po, c, bsize, sym, cap):
    ref = np.zeros(cap + 64, np.uint8)
    po.lib().o_viterbi_decode.restype = C.c_size_t
    n = po.lib().o_viterbi_decode(C.byref(c), bsize, sym.ctypes.data_as(C.c_void_p), C.c_size_t(len(sym)), ref.ctypes.data_as(C.c_void_p))
    return ref[:n]


@pytest.mark.parametrize("const,cr", CONFIGS, ids=IDS)
def test_oracle_decodes_the_clean_inputs(po, const, cr):
    """(no GPU) the oracle alone: on the streams of the sweeps without bit flips it returns the transmitted bytes, at every length"""
    for bsize, lengths in ((48, range(1, 41)), (_small_bsize(const, cr), _small_lengths(const, cr))):
        c, d_nsym, d_nout, data, sym = _stream(po, const, cr, bsize, max(lengths), 0.0)
        for nb in lengths:
            ref = _oracle(po, c, bsize, sym[:nb * d_nsym], nb * d_nout)
            assert len(ref) == max(nb * d_nout - NTB[cr], 0) and (ref == data[:len(ref)]).all(), (bsize, nb)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    return gr_dvbt_amd


@pytest.fixture(scope="module")
def dev():
    import torch

    class Dev:
        s = torch.cuda.Stream()

        def call(self, b, nout, nin, x, out_bytes, tags):
            with torch.cuda.stream(self.s):
                xin = torch.from_numpy(x.copy()).to("cuda")
                out = torch.zeros(out_bytes + 64, dtype=torch.uint8, device="cuda")
            r, cons, _ = b.work_device(nout, nin, xin.data_ptr(), out.data_ptr(), tags, self.s.cuda_stream)
            self.s.synchronize()
            return r, cons, out[:out_bytes].cpu().numpy()
    return Dev()


def _decode(g, dev, const, cr, bsize, sym, d_nsym, d_nout, calls, first_entry=0):
    """the stream through one handle, in calls of calls[i] reference blocks (the last value repeats), host and device entries alternating"""
    b = g.Block("viterbi_decoder", const, 0, cr, bsize, 0, -1)
    outs, pos, k = [], 0, 0
    while pos < len(sym):
        nb = min(calls[min(k, len(calls) - 1)], (len(sym) - pos) // d_nsym)
        tags = [(0, g.TAG_SUPERFRAME_START, 0xaa)] if k == 0 else []
        x = sym[pos:pos + nb * d_nsym]
        if (k + first_entry) % 2 == 0:
            out = np.zeros(nb * d_nout, np.uint8)
            r, cons, _ = b.work(nb * d_nout, nb * d_nsym, np.ascontiguousarray(x), out, tags)
        else:
            r, cons, out = dev.call(b, nb * d_nout, nb * d_nsym, x, nb * d_nout, tags)
        assert cons == nb * d_nsym
        outs.append(out[:r])
        pos += cons
        k += 1
    b.close()
    return np.concatenate(outs)


def _sweep(po, g, dev, const, cr, bsize, lengths):
    c, d_nsym, d_nout, data, sym = _stream(po, const, cr, bsize, max(lengths), _ber(const, cr))
    for nb in lengths:
        ref = _oracle(po, c, bsize, sym[:nb * d_nsym], nb * d_nout)
        got = _decode(g, dev, const, cr, bsize, sym[:nb * d_nsym], d_nsym, d_nout, [nb], first_entry=nb)
        assert len(got) == len(ref) == max(nb * d_nout - NTB[cr], 0), (bsize, nb, len(got), len(ref))
        assert (got == ref).all(), (bsize, nb, np.flatnonzero(got != ref)[:5])
    return c, d_nsym, d_nout, sym


@pytest.mark.gpu
@pytest.mark.parametrize("const,cr", CONFIGS, ids=IDS)
def test_stream_lengths_of_1_to_40_blocks(po, g, dev, const, cr):
    """bsize 48: every length as one call on a fresh handle, then the longest stream in calls of 1, 2, 3 and 5 blocks (the decoder's state is handed from
    call to call at a block of windows, and the call's chunk 0 starts without a warm-up)"""
    c, d_nsym, d_nout, sym = _sweep(po, g, dev, const, cr, 48, range(1, 41))
    ref = _oracle(po, c, 48, sym, 40 * d_nout)
    got = _decode(g, dev, const, cr, 48, sym, d_nsym, d_nout, [1, 2, 3, 5, 1, 1, 2, 5])
    assert len(got) == len(ref) and (got == ref).all(), np.flatnonzero(got != ref)[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("const,cr", CONFIGS, ids=IDS)
def test_stream_end_at_every_place_of_a_block(po, g, dev, const, cr):
    """the smallest legal bsize: 24 consecutive lengths (see the module's docstring)"""
    _sweep(po, g, dev, const, cr, _small_bsize(const, cr), _small_lengths(const, cr))


@pytest.mark.gpu
@pytest.mark.parametrize("const,cr,chunk", [(2, 4, 24), (1, 2, 48)], ids=["qam64-7/8-chunk24", "qam16-3/4-chunk48"])
def test_segment_in_chunks_of_one_and_two_blocks(po, g, const, cr, chunk):
    """the segment API on two 2k superframes with chunks of 24 and 48 bytes: every chunk's bit stream overlays the step words of the chunk before it in the
    wavefront's row, and the best states read at the top of a block are those of a chunk's first and second block.  The oracle receiver's Viterbi tap."""
    c = po.cfg(const, cr, po.T2k)
    ibits = c.payload * c.m * c.k // c.n
    iq = po.tx(c, po.make_ts((272 * ibits * 2) // (204 * 8), 17), lead_in=600, tail=3 * c.N)
    o = po.rx(c, iq, want=("vit",))
    rx = g.Rx(const, cr, po.T2k, max_samples=len(iq), taps=True, viterbi_chunk_bytes=chunk)
    rep = rx.run(iq)
    assert rep.first_out_symbol == o["first_out_symbol"] >= 0
    v = rx.tap(g.TAP_VITERBI).reshape(-1)
    rx.close()
    ref = np.asarray(o["vit"]).reshape(-1)
    assert v.size == ref.size > 0 and (v == ref).all(), np.flatnonzero(v != ref)[:5]
