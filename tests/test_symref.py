"""The float64 demodulator of tests/symref.py, checked on the CPU before tests/test_gpu_symbol_kernels.py holds the symbol kernels to it: against the oracle's own
acquisition -> FFT -> equaliser taps on a clean loopback, for closure on a flat channel, at the edges of the integer-offset search, and -- for every launch of the GPU
test that compares labels -- that the reference itself keeps its carriers away from the decision boundaries (tests/symcases.py builds the launches for both files)."""
import numpy as np
import pytest

import symcases
import symref


@pytest.mark.parametrize("const,cr,mode,nsf", [(1, 0, 0, 2), (2, 4, 1, 2)])
def test_engine_agrees_with_the_oracles_taps_on_a_clean_loopback(po, const, cr, mode, nsf):
    """16 symbols behind first_out_symbol: the oracle's FFT tap through engine() gives its EQ tap within 5e-6 of the spacing (measured: 1.5e-7 for 2k QAM16, 4.2e-7 for
    8k QAM64; the oracle computes in float32), the same integer offset and pattern; its ACQ tap through spectrum64 gives its FFT tap within the chain's 1e-5 of the peak"""
    c = po.cfg(const, cr, mode)
    npk = (272 * (c.payload * c.m * c.k // c.n) * nsf) // (204 * 8)
    iq = po.tx(c, po.make_ts(npk, 11), lead_in=1000, tail=3 * c.N)
    o = po.rx(c, iq, want=("acq", "fft", "eq"), max_sym_taps=330)
    T = symref.Tables(po, c)
    f0 = o["first_out_symbol"]
    assert f0 >= 0 and len(o["eq"]) >= 16 and len(o["fft"]) >= f0 + 16
    for j in range(16):
        X = o["fft"][f0 + j]
        e = symref.engine(T, X)
        assert e["fo"] == o["freq_offset"][f0 + j] == 0 and e["mod"] == o["sym_index"][f0 + j] % 4
        assert symref.worst(o["eq"][j], e["eq"]) <= 5e-6 * T.spacing
        assert np.abs(symref.spectrum64(o["acq"][f0 + j]) - X).max() <= 1e-5 * np.abs(X).max()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("const", [0, 1, 2])
def test_flat_channel_closes_onto_the_transmitted_points(po, mode, const):
    """carrier frames -> samples (complex64) -> reference: every equalised carrier lies on its constellation point.  What is left is the samples' rounding to complex64
    (6e-8 of a sample, averaged over the transform) through a gain interpolated from two pilots: under 2e-6 of the spacing for carriers of at most 3.5 spacings"""
    T, freq = symcases.tables(po, mode, const)
    case = symcases.case(po, mode, f"taps_{const}_flat")
    r = case.ref()
    for s, f in enumerate(symcases.F12):
        _, pay = T.lists(f % 4)
        assert r["mod"][s] == f % 4
        assert symref.worst(r["eq"][s], freq[f][T.zl + pay]) <= 2e-6 * T.spacing
    lab, dist = symref.decide64(T, r["eq"])
    assert symref.worst(r["eq"], T.points[lab]) <= 2e-6 * T.spacing and dist.min() > 0.49
    assert (symref.demap_rule(po, T, r["eq"].astype(np.complex64)) == lab).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_offset_search_at_its_edges_and_on_nothing(po, mode):
    for name in ("taps_2_flat", "taps_2_echo"):
        case = symcases.case(po, mode, name)
        for dt in (np.float64, np.float32):
            r = case.ref(dt)
            assert list(r["fo"]) == [symcases.SHIFTS[i % 4] for i in range(12)]
            assert list(r["mod"]) == [f % 4 for f in symcases.F12]
    T = case.T
    for dt in (np.float64, np.float32):
        e = symref.engine(T, np.zeros(T.N, np.complex64), dt)
        assert (e["fo"], e["mod"]) == (0, 0) and not np.isfinite(e["eq"]).any()


def test_phase_is_the_accumulator_of_the_acquisition():
    """phase64 against the literal statement: the phase advances by incA before each of the first sw samples of the window and by incB before every later one"""
    N, cp = 2048, 64
    for sw in (-1, 0, 1, 31, 127, 129, N - 1, N, N + cp - 1, N + cp, 1 << 30):
        ph, acc = symref.phase64(N, cp, sw, 0.25, 3e-4, -5e-4), 0.25
        for n in range(N):
            acc += 3e-4 if (n + 1 <= sw or not 0 <= sw < N + cp) else -5e-4
            assert abs(ph[n] - acc) < 1e-9, (sw, n)


@pytest.mark.parametrize("const,hier", [(0, 0), (1, 0), (2, 0), (1, 2), (2, 3)])
def test_decide64_is_the_references_rule_away_from_the_boundaries(po, const, hier):
    T, _ = symcases.tables(po, 0, const, hier)
    rng = np.random.RandomState(const + 10 * hier)
    top = np.abs(T.points.real).max() + 5 * T.spacing
    e = (rng.uniform(-top, top, 20000) + 1j * rng.uniform(-top, top, 20000)).astype(np.complex64)
    lab, dist = symref.decide64(T, e)
    far = (dist > 1e-4).all(axis=-1)
    assert far.mean() > 0.99 and (symref.demap_rule(po, T, e)[far] == lab[far]).all()
    assert (symref.decide64(T, T.points)[0] == np.arange(len(T.points))).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_launches_of_the_gpu_test_meet_what_it_relies_on(po, mode):
    """the working bounds are tighter than the project's ceilings (else they would not be working bounds), float32 and float64 find the same offsets and patterns in every
    launch (asserted while the bounds are computed), and in every launch whose labels are compared with decide64 the reference itself puts no more than the allowed
    share of carriers within the margin of a boundary"""
    b = symcases.bounds(po, mode)
    for k, ceil in symcases.CEIL.items():
        assert 0 < b[k] <= 0.6 * ceil, (k, b[k])
    assert b["tps"] <= 1e-4 and b["csi"] <= 1e-4
    for name in symcases.names(mode):
        if not symcases.compares_labels(mode, name):
            continue
        c = symcases.case(po, mode, name)
        _, dist = symref.decide64(c.T, c.ref()["eq"])
        share = float((dist <= b["eq"]).any(axis=-1).mean())
        assert share <= symcases.SHARE_CAP, (name, share)
    e = symcases.case(po, mode, "edge")
    r = e.ref()
    for s in (symcases.EDGE_ZERO, symcases.EDGE_CUT[2]):
        assert (r["fo"][s], r["mod"][s]) == (0, 0) and not np.abs(r["fft"][s]).any()
