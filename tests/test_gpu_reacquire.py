"""A CP lock lost in the middle of a segment.  The reference drops the lock after one missed peak, consumes half a window and searches
again (ofdm_sym_acquisition_impl.cc:545-559); sync_start makes demod_reference_signals hunt the superframe start again (:115-136), the
new superframe_start resets the Viterbi decoder (viterbi_decoder_impl.cc:213-229) and realigns the byte de-interleaver
(convolutional_deinterleaver_impl.cc:109-120), the descrambler re-searches its NSYNC (energy_descramble_impl.cc:121-141).
dvbt_rx_segment_run follows all of it inside the library; the TS must be the oracle's (oracle/o_chain.c), byte for byte, through the gap."""
import numpy as np
import pytest

import gr_dvbt_amd as g

pytestmark = pytest.mark.gpu


def with_gap(po, c, nsf, seed, at_symbol, n_symbols, shift=333):
    iq = po.stream_slice(c, nsf, seed).copy()
    L = c.N + c.cp
    a = po.STREAM_LEAD_IN + at_symbol * L + shift
    iq[a:a + n_symbols * L] = 0
    return iq


@pytest.mark.parametrize("const,cr,mode,nsf,at,n", [
    (g.QAM16, g.C1_2, g.T2k, 6, 272 * 3 + 100, 3),      # a 3-symbol dropout in the middle
    (g.QAM64, g.C7_8, g.T8k, 4, 272 + 250, 3),          # d_fi_start = 2: the second period starts at a frame-3 boundary
    (g.QPSK, g.C2_3, g.T2k, 7, 272 * 2 + 30, 40),       # 40 symbols of silence: calls that find no peak at all in between
])
def test_dropout_in_the_middle_equals_the_oracle(po, const, cr, mode, nsf, at, n):
    c = po.cfg(const, cr, mode)
    iq = with_gap(po, c, nsf, 5, at, n)
    o = po.rx(c, iq, want=("vit", "rs", "ts"))
    assert o["truncated"] == 1 and len(o["ts"]) > 0            # two lock periods delivered items
    rx = g.Rx(const, cr, mode, max_samples=len(iq))
    rep = rx.run(iq)
    assert rep.n_lock_periods == 2 and rep.total_symbols == o["n_acquired"]
    for tap, key in ((g.TAP_VITERBI, "vit"), (g.TAP_RS, "rs"), (g.TAP_TS, "ts")):
        a = rx.tap(tap)
        assert len(a) == len(o[key]) > 0, (key, len(a), len(o[key]))
        assert (a == o[key]).all(), key
    assert rep.rs_fail_words == o["rs_fail"] > 11                  # the junction's words mix two periods: undecodable, passed on as they are
    # the same through the device-pointer entry
    import torch
    dev = torch.from_numpy(iq.view(np.float32)).cuda()
    rep2 = rx.run_device(dev.data_ptr(), len(iq))
    assert rep2.n_lock_periods == 2 and (rx.tap(g.TAP_TS) == o["ts"]).all()
    # ... and the asynchronous entry decodes the first period only and says where the lock ended
    rx.enqueue_device(dev.data_ptr(), len(iq))
    rep3 = rx.finish()
    assert rep3.status & 2 and rep3.resume_sample > 0 and rep3.n_lock_periods == 1
    rx.close()


def gaps(po, c, iq, at_symbols, shift):
    """3 zeroed symbols at each of at_symbols (shift 0: on the symbol grid)"""
    iq = iq.copy()
    L = c.N + c.cp
    for at in at_symbols:
        a = po.STREAM_LEAD_IN + at * L + shift
        iq[a:a + 3 * L] = 0
    return iq


def equals_the_oracle(rx, rep, o, L):
    """the lock periods, the symbol count and the three byte taps of the run that gave `rep`, against the oracle's"""
    assert [(off + fc * L, n) for (off, fc, cp0, n, fo) in rx.lock_periods() if n > 0] == o["lock_periods"]
    assert rep.total_symbols == o["n_acquired"]
    for tap, key in ((g.TAP_VITERBI, "vit"), (g.TAP_RS, "rs"), (g.TAP_TS, "ts")):
        a = rx.tap(tap)
        assert len(a) == len(o[key]), (key, len(a), len(o[key]))
        assert (a == o[key]).all(), key
    if o["first_out_symbol"] < 0:
        assert rep.status & 4 and all(len(o[key]) == 0 for key in ("vit", "rs", "ts"))


# 2k QAM16 1/2, 3 superframes (813 symbols): where the last period that has items is short, a single symbol or missing, and where nothing is delivered --
# whether a period's last item leaves the demodulator depends on a LATER period having items, and that is known only when the later one has been found.
# (gap symbols, shift, lock periods of the oracle, the period looked at, its length, the oracle delivers items)
SHORT_LAST = [
    ((804,), 0, 2, -1, 9, True),             # a short last period behind the first loss
    ((812,), 0, 2, -1, 1, True),             # a last period of a single symbol: acquired, nothing delivered from it
    ((813,), 0, 1, -1, 813, True),           # the lock is lost where the samples run out
    ((300, 804), 0, 3, -1, 9, True),         # three periods, a short last one
    ((300, 809), 0, 3, -1, 4, True),
    ((200, 500, 806), 0, 4, -1, 7, False),   # no period holds a superframe start: nothing delivered
    ((200, 500, 788), 333, 3, 1, 1, False),  # a single-symbol period in the middle, no lock behind the last gap, nothing delivered
]


@pytest.mark.parametrize("at,shift,n_periods,which,length,delivers", SHORT_LAST, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_short_and_single_symbol_periods_equal_the_oracle(po, at, shift, n_periods, which, length, delivers):
    import torch
    c = po.cfg(g.QAM16, g.C1_2, g.T2k)
    L = c.N + c.cp
    iq = gaps(po, c, po.stream_slice(c, 3, 5), at, shift)
    o = po.rx(c, iq, want=("vit", "rs", "ts"))
    assert len(o["lock_periods"]) == n_periods and o["lock_periods"][which][1] == length      # the input is the case it claims to be
    assert (o["first_out_symbol"] >= 0) == delivers and (len(o["ts"]) > 0) == delivers
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=len(iq))
    equals_the_oracle(rx, rx.run(iq), o, L)
    dev = torch.from_numpy(iq.view(np.float32)).cuda()
    equals_the_oracle(rx, rx.run_device(dev.data_ptr(), len(iq)), o, L)
    rx.close()


def test_cut_piece_that_loses_the_lock_says_so(po):
    """a piece of a cut stream (dvbt_rx_set_cut) with a dropout in its middle: every lock period is found, and the report says that
    the piece is laid out from its own start (status bit 7)"""
    from gr_dvbt_amd import multi
    c = po.cfg(g.QAM16, g.C1_2, g.T2k)
    d = g.get_dims(g.QAM16, g.C1_2, g.T2k)
    L = c.N + c.cp
    iq = po.stream_slice(c, 4, 5)
    one = po.rx(c, iq, want=("ts",))
    assert len(one["lock_periods"]) == 1 and one["lock_periods"][0][0] % L == 0 and one["first_out_symbol"] >= 0
    cu = multi.plan_cuts(d, len(iq), 0, one["lock_periods"][0][0] // L + one["first_out_symbol"], 2)[1]
    assert cu["sym_off"] > 0
    piece = iq[cu["begin"]:cu["end"]].copy()
    a = (len(piece) // L // 2) * L                                  # the piece begins on the call grid
    piece[a:a + 3 * L] = 0
    o = po.rx(c, piece, want=("ts",))
    assert len(o["lock_periods"]) == 2 and all(n > 1 for _, n in o["lock_periods"])
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=len(piece))
    rx.set_cut(cu["sym_off"])
    rep = rx.run(piece)
    assert rep.status & 128
    assert [(off + fc * L, n) for (off, fc, cp0, n, fo) in rx.lock_periods() if n > 0] == o["lock_periods"]
    assert rep.total_symbols == o["n_acquired"]
    rx.close()


def test_cut_holds_for_a_later_lock_period_of_the_piece(po):
    """dvbt_rx_set_cut holds for EVERY lock period of a piece walked on its own, not for its first one alone.  2k QAM64 7/8, where two superframes
    are no whole number of Viterbi blocks (544 * 1512 / 1024), so that the block count in the stream's coordinates (viterbi_decoder_impl.cc:198,
    k_backend.hpp plan_body) shows in the byte count; the dropout lies at the piece's fifth symbol, so the period that delivers is the SECOND one."""
    from gr_dvbt_amd import multi
    c = po.cfg(g.QAM64, g.C7_8, g.T2k)
    d = g.get_dims(g.QAM64, g.C7_8, g.T2k)
    L = c.N + c.cp
    iq = po.stream_slice(c, 4, 5)
    one = po.rx(c, iq, want=("ts",))
    assert len(one["lock_periods"]) == 1 and one["lock_periods"][0][0] % L == 0 and one["first_out_symbol"] >= 0
    cu = multi.plan_cuts(d, len(iq), 0, one["lock_periods"][0][0] // L + one["first_out_symbol"], 2)[1]
    piece = iq[cu["begin"]:cu["end"]].copy()
    piece[5 * L:8 * L] = 0
    o = po.rx(c, piece, want=("vit", "ts"))                          # (the oracle knows no cut: the piece as the beginning of a stream)
    assert len(o["lock_periods"]) == 2 and o["lock_periods"][0][1] < 68 < o["first_out_symbol"] and len(o["ts"]) > 0   # the second period delivers
    # the decoder's byte count: whole blocks of 768 bytes' worth of symbols, less the traceback delay -- counted from the piece's superframe start (the oracle) and
    # from the stream's, sym_off symbols earlier (the cut)
    n_out = o["n_acquired"] - 1 - o["first_out_symbol"]
    P, block_syms, block_bytes, sym_bits = d.payload_length, 768 * 8 // 6, 7 * 768 // 8, d.payload_length * 6 * 7 // 8
    delay = (n_out * P // block_syms) * block_bytes - len(o["vit"])
    assert 0 < delay < 64
    want = ((cu["sym_off"] + n_out) * P // block_syms) * block_bytes - cu["sym_off"] * sym_bits // 8 - delay
    assert cu["sym_off"] * P % block_syms != 0 and 0 < want != len(o["vit"])                  # the case can tell the two coordinates apart
    rx = g.Rx(g.QAM64, g.C7_8, g.T2k, max_samples=len(piece))
    rx.set_cut(cu["sym_off"])
    rep = rx.run(piece)
    assert rep.status & 128
    assert [(off + fc * L, n) for (off, fc, cp0, n, fo) in rx.lock_periods() if n > 0] == o["lock_periods"]
    assert rep.total_symbols == o["n_acquired"]
    assert rep.n_viterbi_bytes == want, (rep.n_viterbi_bytes, want, len(o["vit"]))
    assert (rx.tap(g.TAP_VITERBI) == o["vit"][:want]).all()
    ts = rx.tap(g.TAP_TS)
    assert len(ts) == len(o["ts"]) and (ts == o["ts"]).all()
    rx.close()


def test_what_is_delivered_around_the_gap(po):
    """properties: everything the first period could deliver, then the packets of the junction (wrong, as in the reference), then the
    second period from its superframe start on -- all transmitted packets, in order"""
    const, cr, mode, nsf = g.QAM16, g.C1_2, g.T2k, 6
    c = po.cfg(const, cr, mode)
    iq = with_gap(po, c, nsf, 5, 272 * 3 + 100, 3)
    rx = g.Rx(const, cr, mode, max_samples=len(iq))
    rx.run(iq)
    got = rx.tap(g.TAP_TS).reshape(-1, 188)
    rx.close()
    sent = po.stream_ts(c, 0, nsf, 5).reshape(-1, 188)
    idx = {bytes(sent[i]): i for i in range(len(sent))}
    m = np.array([idx.get(bytes(p), -1) for p in got])
    good = m >= 0
    assert good.sum() > 0.9 * len(m)
    assert (np.diff(m[good]) > 0).all()                            # in order, nothing twice
    first_bad = int(np.argmin(good))
    assert m[first_bad - 1] > 504 * 2 and m[np.flatnonzero(good)[-1]] > 504 * 5
    assert (got[:, 0] == 0x47).all()
