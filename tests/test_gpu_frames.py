"""The launches between the symbol kernels and the Viterbi decoder ALONE (dvbt_debug_frames: a test hook of the library that runs launch_frames, the segment path's
own launch block: tps_vote_kernel -> tps_fsm_par_kernel -> tps_tail_kernel -> inner_kernel<6>), where the chain tests reach them only behind a whole acquired stream
whose pattern index advances by one per symbol.  Streams built on the host (tests/framecases.py), every output bit for bit against a model written from the
reference's statements (tests/frameref.py, pinned to the oracle by tests/test_frameref.py): the vote, the symbol indices, first_out, n_out_symbols, status bit 2, the
TPS word, the final members, every size plan_body writes, the de-interleaved rows, and 0xA5 wherever the model says nothing is written.

The fallback flag (trk_flags[9]): asserted 0 where framecases.lanes_off finds every lane's warm-up sufficient (the design's own condition, computed from the stream),
asserted 1 only in the tests whose stream is built to force the fallback and for which lanes_off names a lane; everywhere else only equality with the model.  With -s
every call prints its flag (DESIGN.md section 7 quotes them).

No launch takes a second of GPU time; nothing here provokes a fault (NaN carriers and corrupted words are ordinary data)."""
import ctypes as C

import numpy as np
import pytest

import framecases as fc
import frameref as fr

pytestmark = pytest.mark.gpu

A5 = 0xA5
FILL = 0x3C
SMALL, BIG = 720, 16500                       # calls the two 2k QPSK handles hold
LENGTHS = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 203, 204, 205, 236, 237, 2047, 2048, 2049, 8191, 8192, 8193, 8395, 8396, 8397, 16384, 16385)


class TpsState(C.Structure):
    _fields_ = [("fifo_lo", C.c_uint64), ("fifo_hi", C.c_uint32), ("symbol_index", C.c_int32), ("symbol_index_known", C.c_int32), ("frame_index", C.c_int32),
                ("prev_mod", C.c_int32), ("d_init", C.c_int32)]

    def members(self):
        return (self.fifo_lo, self.fifo_hi, self.symbol_index, self.symbol_index_known, self.frame_index, self.prev_mod, self.d_init)


class Report(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("status", "call0", "cp_start0", "n_symbols", "first_out", "n_out_symbols", "descr_base", "descr_index", "rs_fail", "rs_corr",
                                         "rs_list_n", "small_viol", "drift_known_off", "descr_unclean")] + \
               [(n, C.c_int64) for n in ("n_vit_in", "n_vit_steps", "n_vit_bytes", "n_rs_items", "n_ts_bytes", "sym_off", "n_rs_words", "stream_rs_items", "ts_first_packet")] + \
               [("tps_bits", C.c_uint64)] + [(n, C.c_int32) for n in ("first_cand", "need_seq", "cap_symbols", "has_lp", "has_tap", "reserved")] + [("cap_bytes", C.c_int64)]


ARGTYPES = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_int] + [C.c_void_p] * 7


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _state(st):
    lo, hi, si, known, fi, pm, di = st.members()
    return TpsState(lo, hi, si, known, fi, pm, di)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    gr_dvbt_amd.lib().dvbt_debug_frames.argtypes = ARGTYPES
    return gr_dvbt_amd


class Handle:
    """a receiver handle of `cap` calls with the model's view of its configuration"""

    def __init__(self, g, po, const, rate, mode, cap, hier=0, taps=False, soft=0):
        self.g, self.const, self.rate, self.mode, self.hier, self.cap = g, const, rate, mode, hier, cap
        self.c = po.cfg(const, rate, mode, po.G1_32, hier)
        c = self.c
        self.P, self.m, self.n_tps = c.payload, c.m, c.n_tps
        self.rx = g.Rx(const, rate, mode, max_samples=2 * c.N + c.cp + 16 + (cap - 1) * (c.N + c.cp), hierarchy=hier, taps=taps, soft_decision=soft)
        self.taps = taps
        self.inner = fr.Inner(po, c)
        self.cache = {}
        self.bytes = cap * self.P + 64
        # (a large handle without the LP stream or the tap passes NULL for them; a small one passes arrays, which must come back untouched)
        self.out = {"maj": np.empty(cap, np.int32), "sym_index": np.empty(cap, np.int32), "bitdeint": np.empty(self.bytes, np.uint8),
                    "lp": np.empty(self.bytes, np.uint8) if (hier or cap <= SMALL) else None, "tap": np.empty(self.bytes, np.uint8) if (taps or cap <= SMALL) else None}

    def labels(self, n):
        return fc.labels(n, self.P, self.m)

    def expected_rows(self, rows, sym_index):
        """the de-interleaved rows of the shared labels `rows` under the parity of sym_index: both parities of a row are computed once"""
        need = max(rows) + 1 if len(rows) else 0
        have = self.cache.get("n", 0)
        if need > have and len(rows) <= 64:                            # a few rows of a long stream: no table of every row
            lab = self.labels(need)[np.asarray(rows, np.int64)]
            return list(self.inner.rows(lab, np.asarray(sym_index, np.int64)))
        if need > have:
            n = min(max(need, have * 2, 64), max(self.cap, need))
            lab = self.labels(n)
            self.cache = {"n": n, 0: self.inner.rows(lab, np.zeros(n, np.int64)), 1: self.inner.rows(lab, np.ones(n, np.int64))}
        par = np.asarray(sym_index, np.int64) & 1
        rows = np.asarray(rows, np.int64)
        pick = []
        for j in range(3):
            a0, a1 = self.cache[0][j], self.cache[1][j]
            pick.append(None if a0 is None else np.where(par[:, None] == 1, a1[rows], a0[rows]))
        return pick

    def close(self):
        self.rx.close()


@pytest.fixture(scope="module")
def handles(g):
    import oracle.pyoracle as po
    made = {}

    def get(const=0, rate=0, mode=0, cap=SMALL, hier=0, taps=False, soft=0):
        key = (const, rate, mode, cap, hier, taps, soft)
        if key not in made:
            made[key] = Handle(g, po, const, rate, mode, cap, hier, taps, soft)
        return made[key]

    def drop(h):
        for k, v in list(made.items()):
            if v is h:
                v.close()
                del made[k]
    get.drop = drop
    yield get
    for h in made.values():
        h.close()


def call(H, n_symbols, keep_last, mods, tps, labels, prev0=None, init=None, sym_off=0, delay=0, handle="own", null=()):
    """dvbt_debug_frames; returns (return code, report, final state).  The arrays of H.out are FILL before the call.  handle: another handle's pointer, or None;
    null: names of the arguments to pass as NULL"""
    for a in H.out.values():
        if a is not None:
            a.view(np.uint8)[...] = FILL
    if len(mods) == 0:                                                 # (an empty array has no address to give)
        mods, tps, labels = np.zeros(1, np.int32), np.zeros((1, H.n_tps), np.complex64), np.zeros((1, H.P), np.uint8)
    rep, fin = Report(), TpsState()
    C.memset(C.byref(rep), FILL, C.sizeof(rep))
    C.memset(C.byref(fin), FILL, C.sizeof(fin))
    st = _state(init) if init is not None else None
    a = {"h": H.rx.h if handle == "own" else handle, "mods": _p(np.ascontiguousarray(mods, np.int32)), "tps": _p(np.ascontiguousarray(tps, np.complex64)),
         "prev0": _p(None if prev0 is None else np.ascontiguousarray(prev0, np.complex64)), "init": C.byref(st) if st is not None else None,
         "labels": _p(np.ascontiguousarray(labels, np.uint8)), "rep": C.byref(rep), "maj": _p(H.out["maj"]), "sym_index": _p(H.out["sym_index"]), "fin": C.byref(fin),
         "bitdeint": _p(H.out["bitdeint"]), "lp": _p(H.out["lp"]), "tap": _p(H.out["tap"])}
    a.update({k: None for k in null})
    r = H.g.lib().dvbt_debug_frames(a["h"], n_symbols, keep_last, a["mods"], a["tps"], a["prev0"], a["init"], a["labels"], sym_off, delay, a["rep"], a["maj"],
                                    a["sym_index"], a["fin"], a["bitdeint"], a["lp"], a["tap"])
    return r, rep, fin


FLAGS = {}


def check(H, name, stream, n_symbols=None, keep_last=1, init=None, prev0=None, carried=None, sym_off=0, delay=0, rows="all", force_seq=False, model=None):
    """one call against the model; returns (report, the model's result).  model: the result of an earlier call with the same arguments"""
    n_symbols = stream.n if n_symbols is None else n_symbols
    assert n_symbols <= stream.n and n_symbols <= H.cap
    lab = H.labels(max(n_symbols, 1))
    exp = model if model is not None else fr.run(stream.mods, stream.tps, n_symbols, keep_last, H.const, H.mode, H.rate, H.P, H.m, H.c.k, H.c.n, prev0=prev0, init=init, carried=carried, sym_off=sym_off,
                 start_delay_symbols=delay, snap_every=fc.SEG)
    r, rep, fin = call(H, n_symbols, keep_last, stream.mods[:n_symbols], stream.tps[:n_symbols], lab[:n_symbols], prev0=prev0, init=init, sym_off=sym_off, delay=delay)
    H.g.binding._chk(r)
    ntot, fo, nout = exp["ntot"], exp["first_out"], exp["n_out_symbols"]
    if "off" not in exp:
        exp["off"] = fc.lanes_off(stream, ntot, exp) if prev0 is None else None
    off = exp["off"]
    print(f"FLAG {name}: ntot {ntot} need_seq {rep.need_seq} lanes off {None if off is None else len(off)} first_out {rep.first_out}")
    FLAGS[name] = rep.need_seq
    assert (rep.cap_symbols, rep.cap_bytes, rep.has_lp, rep.has_tap) == (H.cap, H.bytes, 1 if H.hier else 0, 1 if H.taps else 0)
    # the vote and the symbol indices
    maj, si = H.out["maj"], H.out["sym_index"]
    assert (maj[:ntot] == exp["maj"]).all(), (name, np.flatnonzero(maj[:ntot] != exp["maj"])[:8])
    assert (maj[ntot:].view(np.uint8) == A5).all()
    assert (si[:ntot] == exp["sym_index"]).all(), (name, np.flatnonzero(si[:ntot] != exp["sym_index"])[:8])
    assert (si[ntot:].view(np.uint8) == A5).all()
    # the state block
    assert (rep.first_out, rep.n_out_symbols, rep.status) == (fo, nout, 4 if exp["no_start"] else 0), (name, rep.first_out, rep.n_out_symbols, rep.status, fo, nout)
    assert rep.tps_bits == exp["tps_bits"], (name, hex(rep.tps_bits), hex(exp["tps_bits"]))
    for k in ("n_vit_in", "n_vit_steps", "n_vit_bytes", "stream_rs_items", "n_rs_words", "n_rs_items", "sym_off"):
        assert getattr(rep, k) == exp[k], (name, k, getattr(rep, k), exp[k])
    assert (rep.n_symbols, rep.call0, rep.cp_start0, rep.n_ts_bytes, rep.rs_fail, rep.rs_corr, rep.rs_list_n, rep.ts_first_packet) == (n_symbols, 0, 0, 0, 0, 0, 0, 0)
    assert (rep.descr_base, rep.descr_index, rep.small_viol, rep.drift_known_off, rep.descr_unclean) == (0, 0, 0, 0, 0)
    # the members a later period starts from
    assert fin.members() == exp["state"].members(), (name, fin.members(), exp["state"].members())
    # the flag words
    if prev0 is not None:
        assert (rep.first_cand, rep.need_seq) == (fr.NO_CAND, 0)      # a continuation runs no parallel pass: the words stay as the reset left them
    else:
        assert rep.need_seq in (0, 1)
        if not off:
            assert rep.need_seq == 0, (name, "every lane's warm-up suffices, yet the fallback ran")
        if force_seq:
            assert off and rep.need_seq == 1, (name, off[:4], rep.need_seq)
        if rep.need_seq == 0:
            assert rep.first_cand == (fo if fo >= 0 else fr.NO_CAND)
    # the inner stage: rows of the output symbols, 0xA5 behind them
    P = H.P
    for key, j in (("tap", 0), ("bitdeint", 1), ("lp", 2)):
        buf = H.out[key]
        if (key == "tap" and not H.taps) or (key == "lp" and not H.hier):
            assert buf is None or (buf == FILL).all()                  # no such buffer: the caller's array is untouched
            continue
        assert (buf[nout * P:] == A5).all(), (name, key)
        if nout:
            u = np.arange(nout) if rows == "all" else np.unique(np.clip(np.asarray(rows), 0, nout - 1))
            want = H.expected_rows(fo + u, exp["sym_index"][fo + u])[j]
            got = buf[:nout * P].reshape(nout, P)[u]
            assert (got == want).all(), (name, key, np.flatnonzero((got != want).any(1))[:8])
    return rep, exp


def pick(handles, n):
    return handles() if n <= SMALL else handles(cap=BIG)


# ================================================================ lengths and edges of the parallel pass
@pytest.mark.parametrize("ntot", LENGTHS)
def test_every_length_of_a_clean_stream(handles, ntot):
    """ntot symbols reach the bookkeeping, with keep_last 0 (one more acquired) and 1: a lane's first and last symbol, a ragged last dword, the warm-up's length, the
    fallback's tile, a workgroup's edge and the second workgroup's first lanes.  The stream starts 37 symbols in front of a frame 3, so a start lies at symbol 105."""
    for keep in (0, 1):
        n = ntot + (0 if keep else 1)
        H = pick(handles, n)
        rep, exp = check(H, f"length {ntot} keep_last {keep}", fc.clean(n, t0=3 * 68 - 37), keep_last=keep)
        assert exp["first_out"] == (105 if ntot > 105 else -1)


@pytest.mark.parametrize("ntot", (2047, 2048, 2049))
def test_the_fallbacks_tile_edge(handles, ntot):
    """the same lengths on a stream with five corrupted words in a row, which leaves lanes without an intact frame end in their warm-up: the sequential bookkeeping runs,
    over one LDS tile of 2048 symbols and its neighbours"""
    for keep in (0, 1):
        n = ntot + (0 if keep else 1)
        check(handles(cap=BIG), f"fallback length {ntot} keep_last {keep}", fc.fallback_length(n), keep_last=keep, force_seq=True)


@pytest.mark.parametrize("quarter", range(4))
def test_every_start_position_of_a_superframe(handles, quarter):
    """300 symbols from each of the 272 positions of a superframe, frame numbers and pattern phase as transmitted.  Blank counters hold frame 0 and the hunt wants frame
    3, so the superframe start that coincides with symbol 0 (position 0) must NOT fire -- blank counters give a false start there to a hunt on frame 0 only, which a
    shifted piece would be (test_cut_pieces) -- and the stream delivers from symbol 272; a stream that begins later than position 204 holds no whole frame 3 in front
    of its first start: it delivers from its second where the 300 symbols reach it (from position 245 on), else nothing"""
    H = handles()
    for t0 in range(68 * quarter, 68 * quarter + 68):
        rep, exp = check(H, f"start position {t0}", fc.clean(300, t0=t0))
        assert rep.first_out == (272 - t0 if t0 <= 204 else -1 if t0 < 245 else 544 - t0), (t0, rep.first_out)


def test_streams_too_short_for_a_start(handles):
    H = handles()
    for n, t0 in ((0, 0), (1, 0), (2, 271), (67, 205), (68, 204), (135, 137), (300, 210)):
        rep, exp = check(H, f"short {n} from {t0}", fc.clean(n, t0=t0))
        assert (rep.first_out, rep.status & 4, rep.n_out_symbols) == (-1, 4, 0)
        assert (H.out["bitdeint"] == A5).all()


def test_the_earliest_candidate_wins_and_a_later_call_is_not_held_to_it(handles):
    """a long clean stream has a candidate at every superframe start, in many lanes and in all three workgroups: the earliest is the start.  The next call on the same
    handle has its first candidate later than that, and must report its own"""
    H = handles(cap=BIG)
    rep, exp = check(H, "candidates, first at 100", fc.clean(16400, t0=172), rows=(0, 1, 8091, 8092, 16000))
    assert rep.first_out == 100 and rep.first_cand == 100
    rep, exp = check(H, "candidates, first at 250", fc.clean(9000, t0=22), rows=(0, 1, 7941, 7942, 8749))
    assert rep.first_out == 250 and rep.first_cand == 250
    rep, exp = check(H, "candidates, none", fc.clean(200, t0=210))
    assert rep.first_out == -1 and rep.first_cand == fr.NO_CAND


# ================================================================ streams that are not clean
@pytest.mark.parametrize("pos", fc.PLACES)
@pytest.mark.parametrize("kind", fc.KINDS)
def test_one_disturbed_symbol(handles, kind, pos):
    """one wrong pattern index (the symbol and the one behind it see diff 2 and 0, 3 and 3, 0 and 2), one dropped symbol (diff 2), one repeated (diff 0): the closed-form
    FIFO shift for every diff, with either bit inserted (tests/test_frameref.py counts the combinations the set reaches)"""
    s = fc.disturbed(kind, pos)
    check(pick(handles, s.n), f"{kind} at {pos}", s, rows=(0, 1, 50, 5000, 8000))


@pytest.mark.parametrize("place", fc.BAD_PLACES)
@pytest.mark.parametrize("kind", tuple(fc.BAD))
def test_bad_tps_words(handles, kind, place):
    """frames with a flipped TPS bit: one, two in a row, and four and six in a row (more than a lane's warm-up of three frames) near the stream's start, in its middle
    and across symbol 8192"""
    s = fc.bad_words(kind, place)
    check(pick(handles, s.n), f"bad words {kind} {place}", s, rows=(0, 1, 100, 8000), force_seq=kind in ("four", "six"))


@pytest.mark.parametrize("i", range(1, 16))
def test_a_sync_word_with_one_wrong_bit_is_no_sync_word(handles, i):
    """frames 4 and 5 (one of each parity) carry a sync word whose s_i is wrong, with the parity of the word as sent: a code word, but no frame end"""
    s = fc.Stream(range(0, 700), words={4: fc.sync_wrong(4, i), 5: fc.sync_wrong(5, i)})
    rep, exp = check(handles(), f"sync s{i} wrong", s)
    assert not [e for e, _ in exp["valid"] if 4 * 68 <= e < 6 * 68]


def test_sync_word_traps(handles):
    H = handles()
    # s16 is not compared: wrong behind the parity's computation the word matches and fails the check, wrong in front of it the word is accepted
    rep, exp = check(H, "s16 wrong, parity of the right word", fc.Stream(range(0, 700), words={4: fc.sync_wrong(4, 16, reparity=False), 5: fc.sync_wrong(5, 16, reparity=False)}))
    assert not [e for e, _ in exp["valid"] if 4 * 68 <= e < 6 * 68]
    rep, exp = check(H, "s16 wrong, parity of the word sent", fc.Stream(range(0, 700), words={4: fc.sync_wrong(4, 16), 5: fc.sync_wrong(5, 16)}))
    assert [e for e, _ in exp["valid"] if 4 * 68 <= e < 6 * 68] == [5 * 68 - 1, 6 * 68 - 1]
    # the sync pattern inside the parameters: the FIFO is cleared 32 symbols behind the word's end, the next frame end is missed
    # the sync pattern inside the parameters does nothing behind a frame end that cleared the FIFO; behind one that did not (a wrong sync bit, a stream that begins
    # inside a frame) the FIFO's bits 1..15 match 32 symbols late, the check fails, the FIFO is cleared and the next frame end is missed
    rep, exp = check(H, "sync pattern in s33..s47 of a valid word", fc.Stream(range(0, 700), words={4: fc.embedded_sync(4)}))
    assert {5 * 68 - 1, 6 * 68 - 1} <= {e for e, _ in exp["valid"]}
    rep, exp = check(H, "sync pattern in s33..s47 of a word without a frame end", fc.Stream(range(0, 700), words={4: fc.embedded_sync(4, sync_bit=5)}))
    assert not {5 * 68 - 1, 6 * 68 - 1} & {e for e, _ in exp["valid"]} and 7 * 68 - 1 in {e for e, _ in exp["valid"]}
    rep, exp = check(H, "sync pattern in s33..s47 of every word, from inside a frame", fc.Stream(range(20, 720), default=fc.embedded_sync))
    assert rep.first_out == -1 and not exp["valid"]


def test_frame_numbers_that_do_not_count(handles):
    H = handles()
    for name, seq in (("3 3 3 3", (3, 3, 3, 3)), ("0 2 1 3", (0, 2, 1, 3)), ("3 0 0 3 1", (3, 0, 0, 3, 1)), ("1 1 2 2", (1, 1, 2, 2))):
        words = {g: fr.tps_word(g % 2, fc.CELL, frame_bits=((seq[g % len(seq)] >> 1) & 1, seq[g % len(seq)] & 1)) for g in range(12)}
        check(H, f"frame numbers {name}", fc.Stream(range(0, 700), words=words))


def test_negative_votes_at_symbol_0_of_a_frame(handles):
    """symbol 0 carries no TPS bit.  In front of any valid frame its vote goes into the FIFO like every other; behind one (symbol_index known and 0) it is ignored"""
    H = handles()
    for sign in (-1, 1):
        v0 = {g: sign for g in range(12)}
        rep, exp = check(H, f"vote {sign} at symbol 0, every frame", fc.Stream(range(20, 720), vote0=v0))
        assert (exp["maj"][[48, 116, 184]] == sign * 17).all()
        check(H, f"vote {sign} at symbol 0, stale counters", fc.Stream(range(20, 720), vote0=v0, words={3: fc.flipped(3, 31)}))


def test_a_starting_state(handles):
    """the members a piece of a stream starts from (the tps_init path): known counters and a partly filled FIFO, in the lanes whose warm-up begins at symbol 0; the
    lanes behind start blank (sw > 0), most of them in the long stream"""
    full = fc.clean(16000 + 50, t0=130)
    st, _ = fc.state_after(full, 50)
    assert st.symbol_index_known == 0 and any(st.fifo)
    full2 = fc.clean(700 + 150, t0=130)
    st2, _ = fc.state_after(full2, 150)
    assert st2.symbol_index_known == 1 and any(st2.fifo)
    H = handles()
    rep, exp = check(H, "init: part of a word in the FIFO", fc.tail(full2, 50), n_symbols=700, init=fc.state_after(full2, 50)[0])
    whole = fr.run(full2.mods, full2.tps, 750, 1, 0, 0, 0, H.P, H.m, H.c.k, H.c.n)
    assert exp["first_out"] == whole["first_out"] - 50 and (exp["sym_index"] == whole["sym_index"][50:]).all()      # the piece continues the whole stream's run
    check(H, "init: known counters, part of a word", fc.tail(full2, 150), n_symbols=700, init=st2)
    rep, exp = check(H, "init: a chain in stable lock, start at symbol 0", fc.clean(400, t0=272), init=fc.locked_state(272))
    assert rep.first_out == 0 and rep.n_out_symbols == 400
    odd = fr.State([1, 0, 1, 1] * 17, 10, 1, 2, 1, 1)
    check(H, "init: arbitrary members", fc.clean(700, t0=40), init=odd)
    check(H, "init: arbitrary members, short", fc.clean(20, t0=40), init=odd)
    check(H, "init: none of it read at length 0", fc.clean(0), init=odd)
    # a pattern index that never moves leaves the members as they are: the lanes behind the first seven start blank and cannot agree with them
    check(H, "init: a pattern index that never moves", fc.Stream([500] * 300), init=odd, force_seq=True)
    check(handles(cap=BIG), "init: long stream", fc.tail(full, 50), n_symbols=16000, init=st, rows=(0, 1, 15000))


@pytest.mark.parametrize("delay", (0, 1, 67, 68, 271))
def test_cut_pieces(handles, delay):
    """a piece of a cut stream: the hunt fires start_delay_symbols behind a superframe start, in the frame shifted with it, and only on known counters; the sizes in the
    coordinates of a stream whose first start lies sym_off symbols in front"""
    H = handles()
    for sym_off in (0, 272, 272 * 1000):
        rep, exp = check(H, f"cut delay {delay} sym_off {sym_off}", fc.clean(700, t0=150), sym_off=sym_off, delay=delay)
        assert rep.first_out == 272 - 150 + delay
        check(H, f"cut delay {delay} sym_off {sym_off}, known counters", fc.clean(500, t0=272 + delay), sym_off=sym_off, delay=delay, init=fc.locked_state(272 + delay))


def test_the_continuation_branch(handles):
    """prev0 given: sequential bookkeeping alone, DBPSK of symbol 0 against the carriers in front of the gap, the members carried on, the hunt restarted"""
    H = handles()
    full = fc.clean(900, t0=100)
    st, prev = fc.state_after(full, 300)
    st.d_init = 1
    rep, exp = check(H, "continuation from given members", fc.tail(full, 300), n_symbols=500, prev0=prev, init=st)
    assert rep.first_out == 172 + 272 - 300 and exp["state"].d_init == 1
    # the next period carries on from what this one left in the handle
    rep2, exp2 = check(H, "continuation from the handle's members", fc.tail(full, 800), n_symbols=100, prev0=full.tps[799], carried=exp["state"])
    assert rep2.first_out == -1 and exp2["state"].symbol_index == (100 + 899) % 68
    # a gap: the members are stale by 40 symbols, the pattern phase jumps
    check(H, "continuation behind a gap", fc.tail(full, 340), n_symbols=500, prev0=prev, init=st)


CELLS = {"the first lane": (700, 11), "a middle lane": (700, 615), "the last lane": (700, 700), "the second workgroup": (8500, 8500)}


@pytest.mark.parametrize("where", tuple(CELLS))
def test_frames_whose_static_bits_differ(handles, where):
    """a broadcast alternates the two halves of its cell id in s40..s47: the report carries the LAST valid frame's word, as the sequential bookkeeping does, and the same
    on every run"""
    n, ntot = CELLS[where]
    full = fc.Stream(range(0, n + 57), default=fc.cell_words())
    init, _ = fc.state_after(full, 57)                                 # 57 symbols of frame 0 are in the FIFO: its end is symbol 10 of the piece, in the first lane
    s = fc.tail(full, 57)
    H = pick(handles, n)
    seen, exp = set(), None
    for k in range(5):
        rep, exp = check(H, f"cell id, last valid frame in {where}, run {k}", s, n_symbols=ntot, init=init, rows=(0, 1, 7000), model=exp)
        seen.add(rep.tps_bits)
        last = exp["valid"][-1][0]
        assert ntot - 68 <= last < ntot and len(exp["valid"]) == (ntot + 57) // 68
        if len(exp["valid"]) > 1:
            assert fr.static_word(exp["valid"][-1][1]) != fr.static_word(exp["valid"][-2][1])
    assert len(seen) == 1
    cell = sum(((rep.tps_bits >> (40 + j)) & 1) << (7 - j) for j in range(8))
    assert cell == (0x5A if ((ntot + 57) // 68 - 1) % 2 == 0 else 0xC3)


# ================================================================ the vote
@pytest.mark.parametrize("mode", (0, 1))
def test_vote(handles, mode):
    """tps_vote_kernel on random amplitudes (seven decades) and phases: an even split of the carriers (0 must read as bit 0), products that are exactly +0 and -0, a
    symbol of NaNs (that symbol and the next count every carrier negative), with and without carriers in front of symbol 0, at the edges of the kernel's 64 symbols
    per workgroup.  Every other carrier lies 2^-20 of its two products from the boundary (framecases.vote_case; asserted again here)."""
    H = handles(const=2, mode=1, cap=140) if mode else handles()
    k = H.n_tps
    for n in (63, 64, 65, 128, 129):
        for keep in (0, 1):
            for prev in (False, True):
                zeros = (5, [(0, "cancel"), (1, "+0"), (2, "-0"), (k - 1, "cancel")])
                rows, p0, crafted = fc.vote_case(n, k, 100 * n + keep + 2 * prev, tie=9 if k % 2 == 0 else None, zeros=zeros, nan_row=20, prev0=prev)
                assert fr.vote_margin_ok(rows, p0, crafted)
                exp = fr.vote(rows, p0)
                ntot = n if keep else n - 1
                mods = (np.arange(n) % 4).astype(np.int32)
                lab = H.labels(n)
                if prev:
                    r, rep, fin = call(H, n, keep, mods, rows, lab, prev0=p0, init=fr.State())
                else:
                    r, rep, fin = call(H, n, keep, mods, rows, lab)
                H.g.binding._chk(r)
                maj = H.out["maj"]
                assert (maj[:ntot] == exp[:ntot]).all(), (n, keep, prev, np.flatnonzero(maj[:ntot] != exp[:ntot]))
                assert (maj[ntot:].view(np.uint8) == A5).all()
                assert maj[20] == -k and maj[21] == -k
                if k % 2 == 0:
                    assert maj[9] == 0 and exp[9] == 0
                if not prev:
                    assert maj[0] == k
    # 2k: the four lanes of a symbol take 5, 5, 5 and 2 carriers -- a vote that is wrong in the last two alone
    if mode == 0:
        rows, p0, crafted = fc.vote_case(64, k, 77, prev0=True)
        rows[10] = rows[9] * np.float32(2)
        rows[10, 15:] = -rows[10, 15:]
        rows[11] = rows[10] * np.float32(0.5)
        assert fr.vote(rows, p0)[10] == 13 and fr.vote(rows, p0)[11] == 17
        assert fr.vote_margin_ok(rows, p0, crafted)
        r, rep, fin = call(H, 64, 1, (np.arange(64) % 4).astype(np.int32), rows, H.labels(64), prev0=p0, init=fr.State())
        H.g.binding._chk(r)
        assert (H.out["maj"][:64] == fr.vote(rows, p0)).all()


# ================================================================ the sizes
NOUT = (0, 1, 67, 68, 272, 273, 17408)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("const", (0, 1, 2))
def test_sizes(handles, const, mode):
    """plan_body over every constellation, rate and mode, the symbol counts around a frame and a superframe and a long one, at the start of a stream and 1 and 1000
    superframes into it.  The start fires at symbol 0 (a chain in stable lock), so n_out_symbols = ntot; the long count runs on a handle of its own."""
    for rate in range(5):
        for nout in NOUT:
            cap = 280 if nout <= 273 else nout + 2
            H = handles(const=const, rate=rate, mode=mode, cap=cap)
            s = fc.clean(nout, t0=272, mode=mode)
            for sym_off in (0, 272, 272 * 1000):
                rep, exp = check(H, f"sizes {const} {rate} {mode} {nout} {sym_off}", s, init=fc.locked_state(272, fr.fi_start_of(const, mode)), sym_off=sym_off,
                                 rows=(0, 1, nout - 1) if nout > 273 else "all")
                assert rep.n_out_symbols == nout
            if cap > 280:
                handles.drop(H)


def test_sizes_at_the_clamps(handles):
    """plan_body's three clamps -- a negative input / step count, a negative byte count in stream coordinates, a negative word count -- each reached, with the first
    combinations of test_sizes' sweep at which the model says so"""
    reached = [0, 0, 0]
    for j in range(3):
        found = 0
        for const in (0, 1, 2):
            c = handles(const=const, cap=280).c
            for rate, (k, n) in enumerate(((1, 2), (2, 3), (3, 4), (5, 6), (7, 8))):
                for nout in NOUT[:6]:
                    for sym_off in (0, 272, 272 * 1000):
                        if found < 2 and fr.sizes(c.payload, c.m, k, n, rate, nout, sym_off)["clamps"][j]:
                            rep, exp = check(handles(const=const, rate=rate, cap=280), f"clamp {j}: {const} {rate} {nout} {sym_off}", fc.clean(nout, t0=272),
                                             init=fc.locked_state(272), sym_off=sym_off)
                            assert exp["clamps"][j] and rep.n_out_symbols == nout
                            reached[j] += 1
                            found += 1
    assert all(reached), reached


# ================================================================ the inner stage
INNER = {"qpsk 2k": (0, 0, 0), "qam16 2k": (1, 0, 0), "qam64 2k": (2, 0, 0), "qam64 8k": (2, 1, 0), "hier qam16 2k": (1, 0, 2), "hier qam64 2k": (2, 0, 2)}


def _before_a_start(mode, fi, lead, n, kind=None, at=0):
    """n symbols that begin `lead` symbols in front of the symbol at which the hunt fires (frame number fi in front of a frame's first symbol), with the members a chain
    holds there after 204 symbols (known counters, part of a word in the FIFO); kind: a symbol repeated or dropped `at` symbols into the piece"""
    t0 = (544 if fi == 3 else 476) - lead - 204
    full = fc.clean(204 + n, t0=t0, mode=mode) if kind is None else (fc.repeated if kind == "repeat" else fc.dropped)(204 + n, 204 + at, t0=t0, mode=mode)
    return fc.tail(full, 204), fc.state_after(full, 204)[0]


@pytest.mark.parametrize("name", tuple(INNER))
def test_inner_stage(handles, name):
    """inner_kernel<6> on random labels: both de-interleavers with the tap between them, both outputs of a hierarchical mode, from first_out = 0 and from a later
    symbol, and through a repeated symbol inside the output, behind which two symbols in a row are even: the parity is the symbol index's, not the output row's"""
    const, mode, hier = INNER[name]
    H = handles(const=const, mode=mode, hier=hier, cap=140, taps=True)
    fi = fr.fi_start_of(const, mode)
    rep, exp = check(H, f"inner {name} from symbol 0", fc.clean(130, t0=272, mode=mode), init=fc.locked_state(272, fi))
    assert rep.first_out == 0 and rep.n_out_symbols == 130
    # (the pieces begin at a frame's symbol 17, whose TPS bit is 0 in every frame: a fresh period votes its first symbol against zeros, which reads as 0)
    s, init = _before_a_start(mode, fi, 51, 100)
    rep, exp = check(H, f"inner {name} from symbol 51", s, init=init, keep_last=0)
    assert rep.first_out == 51 and rep.n_out_symbols == 48
    s, init = _before_a_start(mode, fi, 51, 100, "repeat", 64)
    rep, exp = check(H, f"inner {name} with a repeated symbol", s, init=init)
    par = exp["sym_index"][rep.first_out:] & 1
    assert rep.first_out == 51 and (par[:-1] == par[1:]).sum() == 1 and (par != (np.arange(len(par)) & 1)).any() and (par != ((np.arange(len(par)) + 1) & 1)).any()
    s, init = _before_a_start(mode, fi, 51, 100, "drop", 65)
    rep, exp = check(H, f"inner {name} with a dropped symbol", s, init=init)
    assert rep.first_out == 51 and rep.n_out_symbols == 49


# ================================================================ refusals
def _device_bytes(g, H, n):
    """the first n bytes of the handle's bit de-interleaver output as they lie on the device (no call of the hook, which would fill the buffer first)"""
    L = g.lib()
    L.dvbt_rx_tap_device_ptr.restype = C.c_void_p
    L.dvbt_rx_tap_device_ptr.argtypes = [C.c_void_p, C.c_int]
    ptr = L.dvbt_rx_tap_device_ptr(H.rx.h, g.binding.TAP_BITDEINT)
    assert ptr
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(n, np.uint8)
    assert hip.hipMemcpy(_p(out), ptr, n, 2) == 0                      # hipMemcpyDeviceToHost
    return out


def test_refusals_leave_everything_untouched(g, handles):
    """every refusal comes before anything is written: the caller's arrays keep their fill, the device's buffers what the call in front left in them"""
    H = handles()
    s = fc.clean(100, t0=200)
    lab = H.labels(100)
    r, rep, fin = call(H, 100, 1, s.mods, s.tps, lab)
    g.binding._chk(r)
    assert rep.n_out_symbols == 28
    before = H.out["bitdeint"].copy()
    assert (_device_bytes(g, H, H.bytes) == before).all()
    soft = handles(soft=1, cap=40)
    bad = [dict(null=(k,)) for k in ("mods", "tps", "labels", "rep", "maj", "sym_index", "fin", "bitdeint")] + [dict(handle=None), dict(handle=soft.rx.h)]
    for kw in (dict(n_symbols=-1), dict(n_symbols=H.cap + 1), dict(sym_off=1), dict(sym_off=271), dict(sym_off=-272), dict(delay=-1), dict(delay=272)):
        bad.append(kw)
    big = fc.clean(H.cap + 1)
    for over in bad:
        a = dict(n_symbols=100, sym_off=0, delay=0)
        a.update({k: over.pop(k) for k in list(over) if k in a})
        r, rep, fin = call(H, max(a["n_symbols"], -1), 1, big.mods, big.tps, H.labels(H.cap + 1), sym_off=a["sym_off"], delay=a["delay"], **over)
        assert r == -1, (a, over)
        assert all((x.view(np.uint8) == FILL).all() for x in H.out.values())
        assert (np.frombuffer(rep, np.uint8) == FILL).all() and (np.frombuffer(fin, np.uint8) == FILL).all()
    assert (_device_bytes(g, H, H.bytes) == before).all()
