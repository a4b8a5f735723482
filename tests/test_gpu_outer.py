"""The outer stage of the segment chain ALONE (dvbt_debug_outer: a test hook of the library), on Viterbi byte streams built on the CPU: the launches
enqueue_tail makes for every segment, piece and lock period -- deint_rs_kernel with its defer list, rs_fix_kernel, descramble_scan_kernel and
descramble_runs_kernel -- and the range form stream_rs_range.  The per-block entries (tests/test_gpu_rx_blocks_sweep.py) run other code, and whole
chains reach this code only on clean loopbacks and a few noise seeds.  Here every path has its own corpus (tests/rxref.py; tests/test_outer_corpus.py
shows that each corpus is what it claims): the last partial wavefront, the junction words among more bad words, the switch between the defer list
and the lane decoder at 23 / 24 bad words, more than 512 deferred words, sync bits patched in both directions, run breaks, dropped items, phase
jumps, more than 8,192 calls in a run, more than 1,024 runs, a piece of a cut stream with its phase check, ranges with history.
The references are the oracle's primitives in sequence and, for a piece, the documented contract.  Every comparison is bit for bit, and what lies
behind the counts in every buffer must still hold the hook's 0xA5."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rxref  # noqa: E402
from rxref import JUNCTION  # noqa: E402

pytestmark = pytest.mark.gpu

SEGMENT, CUT, RANGE = 0, 1, 2
BUF_DEINT, BUF_RS, BUF_TS, BUF_SYNC, BUF_RUNS = range(5)
POISON = 0xA5
MARGIN = 1 << 16


class OuterReport(C.Structure):
    _fields_ = [("n_rs_words", C.c_int64), ("n_rs_items", C.c_int64), ("n_ts_bytes", C.c_int64), ("ts_first_packet", C.c_int64),
                ("cap_bytes", C.c_int64), ("sync_cap_words", C.c_int64), ("runs_cap", C.c_int64),
                ("rs_fail", C.c_int32), ("rs_corr", C.c_int32), ("rs_list_n", C.c_int32), ("n_runs", C.c_int32), ("descr_unclean", C.c_int32),
                ("reserved", C.c_int32)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    L = gr_dvbt_amd.lib()
    L.dvbt_debug_outer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(OuterReport), C.c_void_p, C.c_size_t]
    L.dvbt_debug_outer_read.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_size_t]
    L.dvbt_debug_outer_read.restype = C.c_int64
    return gr_dvbt_amd


def _handle(g, compat):
    return g.Rx(g.QPSK, g.C1_2, g.T2k, max_samples=1 << 16, rs_oracle_compat=compat, taps=True)


@pytest.fixture(scope="module")
def rxs(g):
    """one small handle per decoder setting: 2k QPSK 1/2, the debug taps on (the DEINT tap is written by the fused kernel)"""
    hs = {compat: _handle(g, compat) for compat in (0, 1)}
    yield hs
    for h in hs.values():
        h.close()


def outer(g, rx, mode, stream, a=0, b=0):
    """dvbt_debug_outer; returns (the report, the whole sync bitmap up to its capacity)"""
    rep = OuterReport()
    sync = np.zeros(1 << 16, np.uint64)
    n = 0 if stream is None else len(stream)
    g.binding._chk(g.lib().dvbt_debug_outer(rx.h, mode, None if stream is None else _p(stream), n, a, b, C.byref(rep), _p(sync), len(sync)))
    return rep, sync[:min(len(sync), rep.sync_cap_words)]


def read(g, rx, buf, offset, nbytes):
    out = np.zeros(nbytes, np.uint8)
    n = g.binding._chk(g.lib().dvbt_debug_outer_read(rx.h, buf, offset, _p(out), nbytes))
    return out[:n]


def written_exactly(g, rx, buf, rep, want, what):
    """the buffer's first len(want) bytes are `want`; behind them the poison is intact: up to the capacity of a small handle, over 64 KB of a grown one"""
    want = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    span = rep.cap_bytes if rep.cap_bytes <= (4 << 20) else min(rep.cap_bytes, len(want) + MARGIN)
    got = read(g, rx, buf, 0, span)
    assert len(got) == span >= len(want), what
    wrong = np.flatnonzero(got[:len(want)] != want)
    assert len(wrong) == 0, (what, len(wrong), wrong[:6])
    past = np.flatnonzero(got[len(want):] != POISON)
    assert len(past) == 0, (what, "written behind the count", len(want) + past[:6])


def bitmap_exactly(sync, want, first_word, what):
    assert (sync[first_word:first_word + len(want)] == want).all(), (what, np.flatnonzero(sync[first_word:first_word + len(want)] != want)[:6])
    rest = np.concatenate([sync[:first_word], sync[first_word + len(want):]])
    assert (rest == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), (what, "bitmap written outside its words")


_refs = {}


def reference(po, name, compat, stream=None):
    key = (name, compat)
    if key not in _refs:
        s = rxref.outer_case(po, name)["stream"] if stream is None else stream
        r = rxref.outer_reference(po, s, compat)
        r["runs"], _, _ = rxref.descramble_runs(r["rs"])
        r["stream"] = s
        _refs[key] = r
    return _refs[key]


def check_segment(po, g, rx, compat, name, stream=None, deferred=None):
    """a stream through the segment tail against the oracle: taps, bitmap, counters, the poison behind; returns the report"""
    ref = reference(po, name, compat, stream)
    rep, sync = outer(g, rx, SEGMENT, ref["stream"])
    n = ref["n_words"]
    print(f"OUTER {name} compat {compat}: words {rep.n_rs_words} deferred {rep.rs_list_n} fail {rep.rs_fail} corr {rep.rs_corr} runs {rep.n_runs} ts {rep.n_ts_bytes} "
          f"first {rep.ts_first_packet} | oracle fail {ref['fail']} corr {ref['corr']} runs {len(ref['runs'])} ts {len(ref['ts'])}")
    assert (rep.n_rs_words, rep.n_rs_items) == (n, n // 8), name
    written_exactly(g, rx, BUF_DEINT, rep, ref["deint"], (name, "DEINT"))
    written_exactly(g, rx, BUF_RS, rep, ref["rs"], (name, "RS"))
    bitmap_exactly(sync, ref["bitmap"], 0, name)
    assert (rep.rs_fail, rep.rs_corr) == (ref["fail"], ref["corr"]), name
    if deferred is not None:
        assert rep.rs_list_n == deferred, name
    assert rep.n_ts_bytes == len(ref["ts"]), (name, rep.n_ts_bytes, len(ref["ts"]), rep.n_runs, len(ref["runs"]))
    written_exactly(g, rx, BUF_TS, rep, ref["ts"], (name, "TS"))
    assert rep.ts_first_packet == (ref["runs"][0][0] if ref["runs"] else 0), name
    assert rep.n_runs == len(ref["runs"]), name
    runs = read(g, rx, BUF_RUNS, 0, 24 * rep.n_runs).view(np.int64).reshape(-1, 3)
    dst = 0
    for (src, npk), (src_byte, dst_byte, nbytes) in zip(ref["runs"], runs):
        assert (src_byte, dst_byte, nbytes) == (src * 188, dst, npk * 188), name
        dst += npk * 188
    for tap, want in ((g.TAP_DEINT, n * 204), (g.TAP_RS, n * 188), (g.TAP_TS, len(ref["ts"]))):
        buf = np.zeros(want + 8, np.uint8)
        assert g.lib().dvbt_rx_read_tap(rx.h, tap, _p(buf), len(buf)) == want, (name, tap)
    return rep


def _deferred(po, name):
    c = rxref.outer_case(po, name)
    return rxref.deferred_words(rxref.bad_per_wave(c["nerr"], rxref.segment_words(len(c["stream"]))))


# ---------------------------------------------------------------- segment tail, RS side
@pytest.mark.parametrize("compat", (0, 1))
def test_clean_streams_of_every_small_size(po, g, rxs, compat):
    """16 .. 80 words: one and two wavefronts, the last partial, the scatter's `r < nw + 11` bound; 1,040: 16 whole wavefronts and one of 16 words.
    The 11 junction words fail and go through the defer list, nothing else is touched"""
    for n_out in rxref.CLEAN_SIZES:
        rep = check_segment(po, g, rxs[compat], compat, f"clean-{n_out}", deferred=JUNCTION)
        assert (rep.rs_fail, rep.rs_corr) == (JUNCTION, 0)


@pytest.mark.parametrize("compat", (0, 1))
@pytest.mark.parametrize("load", rxref.LOADS)
def test_bad_words_per_wavefront_across_the_decoder_switch(po, g, rxs, load, compat):
    """1,552 words at 1 .. 64 bad words per wavefront (errors of 1 .. 16 bytes at random places, with byte 0, with byte 203, bursts, parity only, and
    garbage): below 24 the defer list and rs_fix_kernel, from 24 on the lane decoder; at 12 and 13 wavefront 0 with its junction words stands at 23
    and 24; at 23 the list holds more than 512 words (the second trip of rs_fix_kernel's grid)"""
    name = f"load-{load}"
    rep = check_segment(po, g, rxs[compat], compat, name, deferred=_deferred(po, name))
    if load == 23:
        assert rep.rs_list_n > 512


@pytest.mark.parametrize("compat", (0, 1))
def test_defer_list_and_lane_decoder_in_one_launch(po, g, rxs, compat):
    check_segment(po, g, rxs[compat], compat, "cycle", deferred=_deferred(po, "cycle"))


@pytest.mark.parametrize("compat", (0, 1))
def test_bad_words_decode_alike_in_sparse_and_dense_wavefronts(po, g, rxs, compat):
    """the bad words of dense wavefronts (lane decoder) again, 16 to a wavefront among clean words (defer list), and those of sparse wavefronts
    packed 48 to a wavefront: the same payload either way, and the oracle's"""
    for src, per_wave in (("load-25", 16), ("load-12", 48)):
        c = rxref.outer_case(po, src)
        n_out = c["n_out"]
        rx = rxs[compat]
        check_segment(po, g, rx, compat, src)
        first = read(g, rx, BUF_RS, 0, n_out * 188).reshape(-1, 188)
        sel = np.flatnonzero(c["nerr"][:n_out - JUNCTION] != 0)[:per_wave * 20]           # corpus indices
        slots = np.concatenate([rxref.wave_slots(n_out, 1 + k)[:per_wave] for k in range(20)])[:len(sel)]
        corpus = rxref.outer_case(po, "clean-1040")["corpus"]
        corpus = np.concatenate([corpus, corpus[:n_out - len(corpus)]])
        corpus[slots] = c["corpus"][sel]
        moved = rxref.viterbi_stream(po, corpus, 3)
        rep = check_segment(po, g, rx, compat, f"moved-{src}", stream=moved)
        in_wave = np.bincount((slots + JUNCTION) // 64)
        assert rep.rs_list_n == JUNCTION + in_wave[in_wave < rxref.RS_LANE_MIN].sum()
        assert (in_wave >= rxref.RS_LANE_MIN).any() == (per_wave == 48)
        second = read(g, rx, BUF_RS, 0, n_out * 188).reshape(-1, 188)
        assert (second[slots + JUNCTION] == first[sel + JUNCTION]).all()


# ---------------------------------------------------------------- segment tail, sync bits and descrambler
@pytest.mark.parametrize("compat", (0, 1))
def test_every_nsync_phase(po, g, rxs, compat):
    """the NSYNC packets at the output words = p (mod 8): p = 3 .. 7 are found in the first call's search window, p = 0 .. 2 only after two items
    have been dropped"""
    for p in range(8):
        rep = check_segment(po, g, rxs[compat], compat, f"phase-{p}")
        assert rep.ts_first_packet == min(w for w in range(JUNCTION, 32) if w % 8 == p) and rep.n_runs == 1


@pytest.mark.parametrize("compat", (0, 1))
def test_sync_bytes_patched_in_both_directions_by_both_decoders(po, g, rxs, compat):
    """restored NSYNC bytes (atomicOr / the ballot behind the lane decoder) and removed false ones (atomicAnd), each in deferred and in dense
    wavefronts, each on a packet the descrambler examines; uncorrectable words on the call grid break the run as in the oracle.  (With
    rs_oracle_compat = 1 the decoder leaves every word's lowest error, so no sync byte is patched: then the descrambler must follow every one of them)"""
    rep = check_segment(po, g, rxs[compat], compat, "kinds", deferred=_deferred(po, "kinds"))
    assert rep.n_runs == (5 if compat == 0 else len(reference(po, "kinds", 1)["runs"])) >= 5


def test_lost_sync_stretch_and_phase_jumps(po, g, rxs):
    check_segment(po, g, rxs[0], 0, "nosync")
    for k in range(1, 15):
        check_segment(po, g, rxs[0], 0, f"jump-{k}")
    check_segment(po, g, rxs[0], 0, "both")
    check_segment(po, g, rxs[1], 1, "both")


def test_more_runs_than_the_fixed_list_held(po, g):
    """a lost NSYNC on the call grid every three calls, 59,904 words: 1,070 runs.  The reference's descrambler goes on however often it has to search
    again; a run list of 1,024 entries ended the TS there without a word (n_ts_bytes short, no status bit)"""
    rx = _handle(g, 0)
    try:
        rep = check_segment(po, g, rx, 0, "runs")
        assert rep.n_runs > rxref.DESCR_MAX_RUNS and rep.runs_cap >= rep.n_rs_items // 2
    finally:
        rx.close()


def test_one_run_of_more_than_8192_calls(po, g):
    """131,328 words (27 MB of stream): the first run is 8,195 calls long -- the second trip of the scan's load loop finds the break -- and the second
    run starts 8 packets behind the lost NSYNC"""
    rx = _handle(g, 0)
    try:
        rep = check_segment(po, g, rx, 0, "long")
        runs = read(g, rx, BUF_RUNS, 0, 48).view(np.int64).reshape(2, 3)
        assert rep.n_runs == 2 and runs[0, 2] == 8195 * 3008 and runs[1, 0] == (16 + 16 * 8195 + 8) * 188
    finally:
        rx.close()


# ---------------------------------------------------------------- a piece that continues a cut stream
def check_cut(po, g, rx, compat, stream, n, phase16, what):
    ref = rxref.outer_reference(po, stream, compat, n_words=n, descramble=False)
    q, ts, unclean = rxref.cut_reference(po, ref["rs"], phase16)
    rep, sync = outer(g, rx, CUT, stream, n, phase16 + 1)
    assert (rep.n_rs_words, rep.n_rs_items) == (n, n // 8), what
    written_exactly(g, rx, BUF_DEINT, rep, ref["deint"], (what, "DEINT"))
    written_exactly(g, rx, BUF_RS, rep, ref["rs"], (what, "RS"))
    bitmap_exactly(sync, ref["bitmap"], 0, what)
    assert (rep.rs_fail, rep.rs_corr) == (ref["fail"], ref["corr"]), what
    assert (rep.n_ts_bytes, rep.ts_first_packet) == (len(ts), q), what
    written_exactly(g, rx, BUF_TS, rep, ts, (what, "TS"))
    assert rep.descr_unclean == unclean, what
    return rep


@pytest.mark.parametrize("compat", (0, 1))
def test_cut_continuation_clean_at_every_size_and_phase(po, g, rxs, compat):
    """sym_off > 0: n_rs_words of 11 (junction words only) .. 700, none of them the multiple of 16 a segment has; every phase of the whole-stream
    descrambler's calls, and the phase not known: the TS of the contract, descr_unclean = 0"""
    for p in range(16):
        stream = rxref.outer_case(po, f"cut-{p % 8}")["stream"]
        for n in (11, 12, 27, 43, 44, 700):
            rep = check_cut(po, g, rxs[compat], compat, stream, n, p, ("cut", p, n))
            assert rep.descr_unclean == 0
        assert check_cut(po, g, rxs[compat], compat, stream, 700, -1, ("cut", p, "phase unknown")).descr_unclean == 0


def test_cut_continuation_reports_a_call_position_without_its_nsync(po, g, rxs):
    """a call position of the phase inside [11, n - 32] without its NSYNC: descr_unclean = 1 (the streaming entry then sets status bit 64 and follows
    the descrambler itself); the only hit behind n - 32, or the phase another one, or not known: 0"""
    for p in range(16):
        inside = min(w for w in range(200, 232) if w % 16 == p)
        outside = max(w for w in range(700) if w % 16 == p)
        s_in, s_out = rxref.cut_hit(po, p, inside), rxref.cut_hit(po, p, outside)
        assert check_cut(po, g, rxs[0], 0, s_in, 700, p, ("hit", p, inside)).descr_unclean == 1
        assert check_cut(po, g, rxs[0], 0, s_out, 700, p, ("hit", p, outside)).descr_unclean == 0
        assert check_cut(po, g, rxs[0], 0, s_in, 700, (p + 8) % 16, ("hit", p, "other phase")).descr_unclean == 0
        assert check_cut(po, g, rxs[0], 0, s_in, 700, -1, ("hit", p, "phase unknown")).descr_unclean == 0
        assert check_cut(po, g, rxs[0], 0, s_in, inside + 31, p, ("hit", p, "piece ends first")).descr_unclean == 0
        assert check_cut(po, g, rxs[0], 0, s_in, inside + 32, p, ("hit", p, "piece just holds it")).descr_unclean == 1


# ---------------------------------------------------------------- the range form
def check_range(po, g, rx, compat, ref, bad, lo, hi, stream, seen):
    """stream_rs_range over [lo, hi): its RS bytes and bitmap words are the whole stream's, everything else keeps what it held (`seen`: the ranges
    decoded since the upload).  Returns the report"""
    rep, sync = outer(g, rx, RANGE, stream, lo, hi)
    seen = seen + [(lo, hi)]
    want_rs = np.full(rep.cap_bytes, POISON, np.uint8)
    want_sync = np.full(rep.sync_cap_words, 0xA5A5A5A5A5A5A5A5, np.uint64)
    for a, b in seen:
        want_rs[a * 188:b * 188] = ref["rs"][a:b].reshape(-1)
        want_sync[a // 64:(b + 63) // 64] = rxref.sync_bitmap(ref["rs"][a // 64 * 64:b], b - a // 64 * 64)
    got = read(g, rx, BUF_RS, 0, rep.cap_bytes)
    wrong = np.flatnonzero(got != want_rs)
    assert len(wrong) == 0, ((lo, hi), wrong[:6] // 188, wrong[:6] % 188)
    assert (sync == want_sync).all(), ((lo, hi), np.flatnonzero(sync != want_sync)[:6])
    for buf in (BUF_DEINT, BUF_TS):
        assert (read(g, rx, buf, 0, rep.cap_bytes) == POISON).all(), ((lo, hi), buf)
    waves = [bad[w:min(w + 64, hi)].sum() for w in range(lo, hi, 64)]
    assert rep.rs_list_n == rxref.deferred_words(waves), (lo, hi)
    return rep, seen


@pytest.mark.parametrize("compat", (0, 1))
def test_ranges_with_and_without_history(po, g, rxs, compat):
    """2,000 words with both decoders at work: `from` 0 (zero fill in front) and 64, 640 (11 words of history), lengths of 1, 63, 65 and 700 words;
    the bitmap at rs_sync + from / 64; a second range on the same handle starts its own defer list"""
    c = rxref.outer_case(po, "range")
    ref = reference(po, "range", compat)
    assert ref["n_words"] == 2000
    bad = np.ones(2000, bool)
    bad[JUNCTION:] = c["nerr"][:2000 - JUNCTION] != 0
    rx = rxs[compat]
    for lo in (0, 64, 640):
        for n in (1, 63, 65, 700):
            rep, seen = check_range(po, g, rx, compat, ref, bad, lo, lo + n, c["stream"], [])
            _, nf, nc = rxref.rs_decode_words(po, ref["deint"][lo:lo + n], compat)
            assert (rep.rs_fail, rep.rs_corr) == (nf, nc), (lo, n)
            print(f"OUTER range [{lo}, {lo + n}) compat {compat}: deferred {rep.rs_list_n} fail {rep.rs_fail} corr {rep.rs_corr}")
    # the walk's way: range after range over the stream in the handle, the counters carried on
    rep, seen = check_range(po, g, rx, compat, ref, bad, 0, 640, c["stream"], [])
    assert rep.rs_list_n > 0
    for lo, hi in ((640, 1340), (1344, 1345), (1408, 2000)):
        rep, seen = check_range(po, g, rx, compat, ref, bad, lo, hi, None, seen)
    total = [rxref.rs_decode_words(po, ref["deint"][a:b], compat)[1:] for a, b in seen]
    assert (rep.rs_fail, rep.rs_corr) == tuple(np.sum(total, axis=0))


# ---------------------------------------------------------------- what the hook refuses
def test_hook_refuses_what_the_tail_could_not_be_given(g, rxs):
    L, rx = g.lib(), rxs[0]
    rep = OuterReport()
    s = np.zeros(204 * 64, np.uint8)
    for mode, n, a, b in ((SEGMENT, -1, 0, 0), (SEGMENT, (1 << 30) + 1, 0, 0), (3, len(s), 0, 0), (-1, len(s), 0, 0), (CUT, len(s), 65, 0), (CUT, len(s), -1, 0),
                          (CUT, len(s), 64, 17), (CUT, len(s), 64, -1), (RANGE, len(s), 32, 64), (RANGE, len(s), 0, 65), (RANGE, len(s), 64, 0), (RANGE, len(s), -64, 0)):
        assert L.dvbt_debug_outer(rx.h, mode, _p(s), n, a, b, C.byref(rep), None, 0) == -1, (mode, n, a, b)
    assert L.dvbt_debug_outer(rx.h, SEGMENT, None, len(s), 0, 0, C.byref(rep), None, 0) == -1
    assert L.dvbt_debug_outer(None, SEGMENT, _p(s), len(s), 0, 0, C.byref(rep), None, 0) == -1
    assert L.dvbt_debug_outer(rx.h, SEGMENT, _p(s), len(s), 0, 0, None, None, 0) == -1
    out = np.zeros(8, np.uint8)
    assert L.dvbt_debug_outer_read(rx.h, 9, 0, _p(out), 8) < 0 and L.dvbt_debug_outer_read(rx.h, BUF_RS, -1, _p(out), 8) == -1
    assert L.dvbt_debug_outer(rx.h, SEGMENT, _p(s), 0, 0, 0, C.byref(rep), None, 0) == 0 and (rep.n_rs_words, rep.n_ts_bytes, rep.rs_list_n) == (0, 0, 0)
