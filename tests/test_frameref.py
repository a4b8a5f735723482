"""tests/frameref.py (the model tests/test_gpu_frames.py compares the frame bookkeeping and the inner stage with) pinned to the oracle, on the CPU: the symbol
indices, the superframe start and first_out against the whole receive chain on clean loopbacks that begin anywhere in a superframe; the sizes against the lengths of
the oracle's Viterbi and RS taps, at the start of a stream and as a piece of a cut one; the BCH check and the word builder against o_bch_check / o_tps_format.  And
the inputs of the GPU test: the vote cases meet their margin, the disturbed streams reach every (shift, inserted bit) the closed-form FIFO shift has, the streams meant
to force the sequential fallback do leave a lane without the sequential members, and framecases.lanes_off's short cut changes nothing."""
import ctypes as C

import numpy as np
import pytest

import framecases as fc
import frameref as fr


@pytest.fixture(scope="module")
def po():
    import oracle.pyoracle as po
    po.lib()
    return po


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _oracle_words(po, c):
    wk = np.zeros(c.Kmax + 1, np.int8)
    po.lib().o_prbs_wk(C.byref(c), _p(wk))
    words = []
    for f in range(4):
        t = np.zeros(68, np.uint8)
        po.lib().o_tps_format(C.byref(c), f, _p(wk), _p(t))
        words.append([int(b) for b in t])
    return words


@pytest.mark.parametrize("mode,const,begins", [(0, 0, (0, 1, 67, 68, 150, 203, 204, 205, 271)), (1, 2, (0, 100, 210))])
def test_bookkeeping_against_the_oracle_chain(po, mode, const, begins):
    """clean loopbacks that begin `begin` symbols into a superframe: the model, fed the true pattern indices and the DBPSK of o_tps_format's frames, gives the
    chain's symbol indices, its first superframe start and first_out_symbol"""
    c = po.cfg(const, po.C1_2, mode)
    L = c.N + c.cp
    words = _oracle_words(po, c)
    for f in range(4):
        assert fr.bch_check(words[f]) == 0 and fr.tps_word(f, {i: words[f][i] for i in range(25, 54)})[1:] == words[f][1:]
    n_sym = 330 if mode == 0 else 140
    for b in begins:
        begin = po.STREAM_LEAD_IN + b * L + L // 3
        iq = po.stream_slice(c, 3, 11, begin=begin, end=begin + n_sym * L)
        o = po.rx(c, iq, want=(), max_sym_taps=4)
        nacq = o["n_acquired"]
        assert nacq >= n_sym - 3
        # the true symbol of acquired item 0, from where its FFT window begins in the stream
        t0 = (begin + int(o["call_pos"][0]) + int(o["cp_start"][0]) - c.N + 1 - po.STREAM_LEAD_IN) // L
        assert t0 in (b, b + 1)
        s = fc.Stream(range(t0, t0 + nacq), mode=mode, default=lambda g, w=words: w[g % 4])
        exp = fr.run(s.mods, s.tps, nacq, 0, const, mode, 0, c.payload, c.m, c.k, c.n)
        assert (exp["sym_index"] == o["sym_index"][:nacq - 1]).all(), b
        sf = np.flatnonzero(o["sf_flag"][:nacq - 1] == 1)
        assert exp["first_out"] == o["first_out_symbol"] and (exp["first_out"] == (sf[0] if len(sf) else -1)), (b, exp["first_out"], o["first_out_symbol"])
        assert (np.flatnonzero(exp["flags"] == 2) == sf).all() and ((exp["flags"] != 0) == (o["sf_flag"][:nacq - 1] != 0)).all()


@pytest.mark.parametrize("rate", range(5))
def test_sizes_against_the_oracles_taps(po, rate):
    """n_vit_bytes and n_rs_words are the lengths of the oracle's Viterbi and RS taps, for a stream's beginning and for a piece 1 and 7 superframes into a cut stream"""
    c = po.cfg(po.QPSK, rate, po.T2k)
    L = c.N + c.cp
    iq = po.stream_slice(c, 3, 5, begin=0, end=po.STREAM_LEAD_IN + 600 * L)
    for sym_off in (0, 272, 272 * 7):
        o = po.rx(c, iq, want=("vit", "rs", "bitdeint"), sym_off=sym_off)
        nout = len(o["bitdeint"])
        assert nout > 300
        z = fr.sizes(c.payload, c.m, c.k, c.n, rate, nout, sym_off)
        assert z["n_vit_bytes"] == len(o["vit"]) and z["n_rs_words"] * 188 == len(o["rs"]), (rate, sym_off, z, len(o["vit"]), len(o["rs"]))
        assert z["stream_rs_items"] == o["stream_rs_items"]


def test_bch_and_word_builder_against_the_oracle(po):
    L = po.lib()
    rng = np.random.RandomState(3)
    for trial in range(300):
        fields = {i: int(rng.randint(2)) for i in range(17, 54)}
        w = fr.tps_word(trial % 4, fields, frame_bits=(int(rng.randint(2)), int(rng.randint(2))))
        for flips in (0, 1, 2):
            v = np.array(w, np.uint8)
            for i in rng.choice(np.arange(1, 68), flips, replace=False):
                v[i] ^= 1
            assert fr.bch_check(list(v)) == L.o_bch_check(_p(v)) == (0 if flips == 0 else -1)
        v = rng.randint(0, 2, 68).astype(np.uint8)
        assert fr.bch_check(list(v)) == L.o_bch_check(_p(v))
        assert fr.static_word(w) >> 63 == 1 and all(((fr.static_word(w) >> i) & 1) == w[i] for i in fr.STATIC_BITS) and fr.static_word(w) & (3 << 23) == 0


def test_vote_cases_meet_the_margin():
    """what tests/test_gpu_frames.py::test_vote feeds the kernel: every carrier outside the crafted zeros and NaNs lies 2^-20 of its two products from the boundary"""
    for k in (17, 68):
        for n in (63, 64, 65, 128, 129):
            for keep in (0, 1):
                for prev in (False, True):
                    zeros = (5, [(0, "cancel"), (1, "+0"), (2, "-0"), (k - 1, "cancel")])
                    rows, p0, crafted = fc.vote_case(n, k, 100 * n + keep + 2 * prev, tie=9 if k % 2 == 0 else None, zeros=zeros, nan_row=20, prev0=prev)
                    assert fr.vote_margin_ok(rows, p0, crafted)
                    assert not fr.vote_margin_ok(rows, p0, None)          # (the crafted ones do not meet it: the check sees them)
                    maj = fr.vote(rows, p0)
                    assert maj[20] == -k and maj[21] == -k and (k % 2 or maj[9] == 0)
                    re, _ = fr.vote_re(rows, p0)
                    assert re[5, 0] == 0 and re[5, 1] == 0 and re[5, 2] == 0 and np.signbit(re[5, 2]) and not np.signbit(re[5, 1])
    for s in (fc.clean(700, t0=3), fc.dropped(700, 40), fc.repeated(700, 41)):
        assert fr.vote_margin_ok(s.tps[1:], s.tps[0])


def _shifts(stream):
    """(diff, inserted bit) of every symbol, as the model walks the stream"""
    maj = fr.vote(stream.tps)
    st, seen, known = fr.State(), set(), 0
    for s in range(stream.n):
        diff = (int(stream.mods[s]) - st.prev_mod + 4) % 4
        si = (st.symbol_index + diff) % 68
        bit = (0 if maj[s] >= 0 else 1) if (not st.symbol_index_known or si != 0) else 0
        seen.add((diff, bit))
        fr.bookkeeping(stream.mods[s:s + 1], maj[s:s + 1], 1, st)
    return seen


def test_disturbed_streams_reach_every_shift():
    seen = set()
    for kind in fc.KINDS:
        for pos in fc.PLACES[:6]:
            seen |= _shifts(fc.disturbed(kind, pos))
    assert seen >= {(d, b) for d in (0, 1, 2, 3) for b in (0, 1)}, seen


def _model(s, n=None, keep=1, init=None):
    n = s.n if n is None else n
    return fr.run(s.mods, s.tps, n, keep, 0, 0, 0, 1512, 2, 1, 2, init=init, snap_every=fc.SEG)


def test_lanes_off():
    """the streams built to force the fallback leave a lane without the sequential members; clean ones leave none; the short cut agrees with the full walk"""
    for n in (2047, 2048, 2049):
        s = fc.fallback_length(n)
        e = _model(s)
        assert fc.lanes_off(s, n, e)
    for kind in ("four", "six"):
        for place in fc.BAD_PLACES[:2]:
            s = fc.bad_words(kind, place)
            e = _model(s)
            assert fc.lanes_off(s, s.n, e), (kind, place)
    cases = [fc.clean(2100, t0=167), fc.clean(700, t0=5)] + [fc.disturbed(k, p) for k in fc.KINDS for p in fc.PLACES[:6]] + \
            [fc.bad_words(k, p) for k in fc.BAD for p in fc.BAD_PLACES[:2]] + [fc.Stream(range(0, 700), words={4: fc.embedded_sync(4)})]
    for s in cases:
        e = _model(s)
        assert fc.lanes_off(s, s.n, e, quick=True) == fc.lanes_off(s, s.n, e, quick=False)
    assert not fc.lanes_off(cases[0], 2100, _model(cases[0])) and not fc.lanes_off(cases[1], 700, _model(cases[1]))


def test_sizes_reach_every_clamp():
    """the sweep of tests/test_gpu_frames.py::test_sizes reaches a negative input count, a negative byte count in stream coordinates and a negative word count, in 2k
    (where test_sizes_at_the_clamps looks for them); no size is ever negative"""
    for payload in (1512, 6048):
        hit = [0, 0, 0]
        for m in (2, 4, 6):
            for rate, (k, n) in enumerate(((1, 2), (2, 3), (3, 4), (5, 6), (7, 8))):
                for nout in (0, 1, 67, 68, 272, 273, 17408):
                    for sym_off in (0, 272, 272000):
                        z = fr.sizes(payload, m, k, n, rate, nout, sym_off)
                        for j in range(3):
                            hit[j] += z["clamps"][j]
                        assert min(z["n_vit_in"], z["n_vit_steps"], z["n_vit_bytes"], z["n_rs_words"], z["stream_rs_items"]) >= 0
        assert all(hit), (payload, hit)
