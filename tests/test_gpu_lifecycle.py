"""Creation, reconfiguration and destruction of every handle of the C ABI.  Every device buffer, page-locked block, stream and event of a handle is a member
of owner type (gr_dvbt_amd/csrc/hip_own.hpp) and is released by the handle's destructor; these cases walk the paths on which members come and go while the handle
lives -- the debug taps switched on and off, a stream object with four chains built twice, every create function refused once and then used three times over --
and require the decoded bytes to stay what they were.  2k QPSK 1/2, guard 1/32, two superframes of loopback signal.  (Allocation failures are not provoked on
the GPU: tests/test_hip_own_host.py runs those paths against counting stubs.)"""
import ctypes as C

import numpy as np
import pytest

import gr_dvbt_amd as g

pytestmark = pytest.mark.gpu

CONST, CR, MODE = g.QPSK, g.C1_2, g.T2k


@pytest.fixture(scope="module")
def signal(po):
    """(samples, the oracle's TS of them): shared by the cases, never written to"""
    c = po.cfg(CONST, CR, MODE)
    iq = po.tx(c, po.make_ts(252 * 2, 1), lead_in=1000, tail=3 * c.N)          # 252 packets fill a superframe of 2k QPSK 1/2
    ref = po.rx(c, iq, want=("ts",))["ts"].copy()
    assert len(ref) > 0
    iq.setflags(write=False); ref.setflags(write=False)
    return iq, ref


def _taps(rx, n):
    assert rx.L.dvbt_rx_enable_taps(rx.h, n) == 0, rx.L.dvbt_last_error()


def _run(rx, iq):
    rx.run(iq)
    return rx.tap(g.TAP_TS).copy()


def test_rx_taps_on_and_off(signal):
    iq, ref = signal
    rx = g.Rx(CONST, CR, MODE, max_samples=len(iq))
    runs = [_run(rx, iq)]
    for n in (1, 0, 2, 0):
        _taps(rx, n)
        runs.append(_run(rx, iq))
    rx.close()
    for ts in runs:
        assert len(ts) == len(ref) and (ts == ref).all()


def test_rx_soft_decision_keeps_eq_when_taps_go(signal):
    """in soft-decision mode `eq` is the soft demapper's input, not a debug tap: switching the taps off must leave it (dvbt_rx_enable_taps)"""
    iq, ref = signal
    rx = g.Rx(CONST, CR, MODE, max_samples=len(iq), soft_decision=1)
    _taps(rx, 0)
    ts = _run(rx, iq)
    rx.close()
    assert len(ts) == len(ref) and (ts == ref).all()             # a clean signal: soft and hard decisions decode the same bytes


def test_rx_stream_built_twice(signal):
    iq, _ = signal
    outs = []
    for _ in range(2):
        st = g.RxStream(CONST, CR, MODE, chains=4)
        st.push(iq[:len(iq) // 3]); st.push(iq[len(iq) // 3:])
        st.finish()
        outs.append(st.pull())
        st.close()
    assert len(outs[0]) > 0 and len(outs[0]) % 188 == 0
    assert len(outs[1]) == len(outs[0]) and (outs[1] == outs[0]).all()


def test_tx_refused_then_three_times():
    with pytest.raises(g.DvbtError, match="error -1"):
        g.Tx(CONST, CR, MODE, scale=0.0)
    ts = np.zeros(188, np.uint8); ts[0] = 0x47
    first = None
    for _ in range(3):
        tx = g.Tx(CONST, CR, MODE, max_packets=8)
        out = tx.run(ts)
        tx.close()
        first = out if first is None else first
        assert len(out) == len(first) and (out.view(np.uint32) == first.view(np.uint32)).all()


P, N = 1512, 2048                                                # payload carriers and FFT length of the 2k mode
# name: (a parameter set the create function refuses with DVBT_ERR_INVALID -- None: it refuses none, a null params pointer then --, a valid one, the smallest call:
# noutput_items, ninput_items (None: what forecast says), tags)
BLOCKS = {
    "ofdm_sym_acquisition": ((2, N, 1705, 64, 30.0), (1, N, 1705, 64, 30.0), 1, None, ()),
    "fft": ((1000, 1, 1), (N, 1, 1), 1, 1, ()),
    "demod_reference_signals": ((4, N, P, 0, 0, 0, 0, 0, 0, 0, 0), (8, N, P, 0, 0, 0, 0, 0, 0, 0, 0), 1, 2, ((0, g.TAG_SYNC_START, 1),)),
    "demap": ((0, 0, 0, 0, 1.0), (P, 0, 0, 0, 1.0), 1, 1, ()),
    "symbol_inner_interleaver": ((100, 0, 0), (P, 0, 0), 1, 1, ((0, g.TAG_SYMBOL_INDEX, 0),)),
    "bit_inner_deinterleaver": ((100, 0, 0, 0), (P, 0, 0, 0), 1, 1, ()),
    "viterbi_decoder": ((0, 0, 0, 0, 0, -1), (0, 0, 0, 768, 0, -1), 96, 768, ((0, g.TAG_SUPERFRAME_START, 0xaa),)),
    "convolutional_deinterleaver": ((100, 12, 17), (136, 12, 17), 2, 2 * 1632, ()),
    "reed_solomon_dec": ((2, 8, 0x11d, 255, 223, 16, 0, 8, 0), (2, 8, 0x11d, 255, 239, 8, 51, 8, 0), 1, 1, ()),
    "energy_descramble": (None, (8,), 4 * 1504, 4, ()),
    "resampler": ((0, 70, 1.0), (64, 70, 1.0), 16, 16, ()),
    "energy_dispersal": ((0,), (1,), 1, 1504, ()),
    "reed_solomon_enc": ((2, 8, 0x11d, 255, 223, 16, 0, 8), (2, 8, 0x11d, 255, 239, 8, 51, 1), 1, 1, ()),
    "convolutional_interleaver": ((0, 12, 17), (136, 12, 17), 12 * 136, 1, ()),
    "inner_coder": ((2, P, 0, 0, 0), (1, P, 0, 0, 0), 4, None, ()),
    "bit_inner_interleaver": ((P, 2, 1, 0), (P, 0, 0, 0), 1, 1, ()),
    "map": ((0, 0, 0, 0, 1.0), (P, 0, 0, 0, 1.0), 1, 1, ()),
    "reference_signals": ((4, P, N, 0, 0, 0, 0, 0, 0, 0, 0), (8, P, N, 0, 0, 0, 0, 0, 0, 0, 0), 1, 1, ()),
}


def test_every_block_has_a_row():
    assert set(BLOCKS) == set(g.BLOCK_PARAMS)


@pytest.mark.parametrize("blk", sorted(BLOCKS))
def test_block_refused_then_three_times(blk):
    bad, good, nout, nin, tags = BLOCKS[blk]
    create = getattr(g.lib(), f"dvbt_{blk}_create")
    create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    p = g.BLOCK_PARAMS[blk](*bad) if bad is not None else None
    assert create(C.byref(p) if p is not None else None, C.byref(h)) == -1
    assert not h.value
    # zeros in, room to spare on both sides: no item of these calls is larger than an FFT item of 16 KB, none takes more than a few of them
    inp, first = np.zeros(1 << 20, np.uint8), None
    for _ in range(3):
        b = g.Block(blk, *good)
        out = np.full(1 << 20, 0xEE, np.uint8)
        r, cons, _ = b.work(nout, b.forecast(nout) if nin is None else nin, inp, out, tags=list(tags))
        b.close()
        assert r >= 0 and cons >= 0
        first = (r, cons, out) if first is None else first
        assert (r, cons) == first[:2] and (out == first[2]).all()
