"""The spectrum analyser's model (tests/specref.py) against closed forms, and the Python helpers of gr_dvbt_amd.SpectrumReading against the model's.  No GPU."""
import numpy as np
import pytest

import rfref as rr
import specref as sr

FS = sr.SAMPLE_RATE
HB = 1705 * FS / 2048 / 2                          # half the occupied bandwidth of an 8 MHz DVB-T signal: 3.805 MHz


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    return gr_dvbt_amd


@pytest.mark.parametrize("kind", [sr.RECT, sr.HANN, sr.BH4])
def test_an_on_bin_tone_reads_its_power_over_the_enbw(kind):
    N, A, b0 = 256, 0.75, 37
    x = (A * np.exp(2j * np.pi * b0 * np.arange(40 * N) / N)).astype(np.complex64)
    r = sr.welch(x, N, N // 2, kind)
    assert r.segments == 79
    assert r.psd[N // 2 + b0] == pytest.approx(A * A / sr.enbw(N, kind), rel=1e-6)
    assert int(np.argmax(r.psd)) == N // 2 + b0
    assert sr.enbw(N, sr.RECT) == 1.0 and sr.enbw(N, sr.HANN) == pytest.approx(1.5, rel=1e-6) and sr.enbw(N, sr.BH4) == pytest.approx(2.0044, rel=1e-4)


def test_windows_are_periodic_float_tables():
    for kind in (sr.HANN, sr.BH4):
        w = sr.window(64, kind)
        assert w.dtype == np.float32 and w[32] == pytest.approx(1.0, abs=1e-6) and np.allclose(w[1:], w[1:][::-1], rtol=0, atol=1e-7)
    assert sr.window(64, sr.HANN)[0] == 0.0 and sr.window(64, sr.BH4)[0] == pytest.approx(6e-5, abs=1e-7)


@pytest.fixture(scope="module")
def noise():
    rng = np.random.RandomState(3)
    return ((rng.randn(1 << 20) + 1j * rng.randn(1 << 20)) * np.sqrt(0.5)).astype(np.complex64)


@pytest.mark.parametrize("kind", [sr.RECT, sr.HANN, sr.BH4])
def test_the_psd_of_white_noise_adds_up_to_the_mean_power(noise, kind):
    r = sr.welch(noise[:1 << 18], 1024, 512, kind)
    assert r.segments >= 256
    assert r.psd.sum() == pytest.approx(r.mean_power, rel=1e-3)
    assert r.mean_power == pytest.approx(1.0, rel=1e-2)


def test_the_binning_by_float_bits():
    p = np.array([1.0, 1.09, 1.999, 2.0, 0.5], np.float32)
    assert list(sr.bins_of(p)) == [1016, 1016, 1023, 1024, 1008]
    assert list(sr.bins_of(np.array([0.0, np.inf, np.nan, -np.nan], np.float32))) == [0, 2040, 2044, 2044]
    x = np.array([1 + 0j, 0.6 + 0.8j, 1 + 1j, 3e-23 + 0j, np.inf + 1j, np.nan + 0j], np.complex64)
    assert list(sr.bins_of(sr.power32(x))[[0, 2, 4, 5]]) == [1016, 1024, 2040, 2044]
    # power32 is fmaf(re, re, im im): against exact rational arithmetic
    from fractions import Fraction
    rng = np.random.RandomState(8)
    z = (rng.randn(2000) * 10.0 ** rng.uniform(-3, 3, 2000) + 1j * rng.randn(2000) * 10.0 ** rng.uniform(-3, 3, 2000)).astype(np.complex64)
    got = sr.power32(z)
    for v, p in zip(z, got):
        im2 = Fraction(float(np.float32(v.imag) * np.float32(v.imag)))
        exact = Fraction(float(v.real)) ** 2 + im2
        lo, hi = np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(np.inf))
        assert abs(Fraction(float(p)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


def test_the_ccdf_of_gaussian_samples_is_exponential(noise):
    r = sr.welch(noise, 2048, 2048, sr.RECT)
    assert r.samples_counted == 1 << 20
    lev, p = r.ccdf()
    for t_db in (4.0, 6.0):
        got = float(np.interp(t_db, lev, p))                   # bin edges are 0.376 dB apart
        assert got == pytest.approx(np.exp(-10 ** (t_db / 10)), rel=0.05), t_db
    assert abs(r.papr_db(np.exp(-10 ** 0.6)) - 6.0) <= 0.05
    assert r.papr_db() == pytest.approx(10 * np.log10(float(r.peak_power) / r.mean_power))
    assert 10.0 < r.papr_db() < 13.0


def _brick(N=1024, floor=1e-4):
    """a brick-wall PSD: 1 per bin over |f| <= HB, `floor` elsewhere, with one louder bin on each side in the shoulder's range"""
    f = (np.arange(N) - N // 2) * FS / N
    psd = np.where(np.abs(f) <= HB, 1.0, floor)
    up, dn = int(np.argmin(np.abs(f - (HB + 500e3)))), int(np.argmin(np.abs(f + (HB + 400e3))))
    psd[up], psd[dn] = 1e-3, 1e-2
    hist = np.zeros(sr.HIST_BINS, np.uint64)
    hist[1016], hist[1024], hist[1040] = 900, 90, 10
    return f, psd, hist


def _both(g, psd, hist, N=1024):
    args = (psd, hist, 10, 1100, 1000, 0, 1500.0, 9.5, N, 100, sr.HANN)
    return sr.Reading(*args), g.SpectrumReading(*args)


def test_shoulder_and_occupied_bandwidth_of_a_brick_wall(g):
    f, psd, hist = _brick()
    for r in _both(g, psd, hist):
        lower, upper = r.shoulder_db(HB)
        assert lower == pytest.approx(20.0, abs=1e-9) and upper == pytest.approx(30.0, abs=1e-9)
        nb = int((np.abs(f) <= HB).sum())                  # 853 bins hold all but 1.1e-2 + 170e-4 of 853
        want = next(k for k in range(1, 1025, 2) if k >= 0.5 * psd.sum())                # the band's bins are all 1: the smallest odd count that is half of it
        assert r.occupied_bandwidth(0.5) == want * FS / 1024
        assert r.occupied_bandwidth(0.95) <= nb * FS / 1024 < r.occupied_bandwidth(0.99999)
        assert r.band_power(-HB, HB) == pytest.approx(nb)
        with pytest.raises(ValueError):
            r.shoulder_db(HB, 300e3, 800e3)                # 3.805 + 0.8 MHz lies beyond Nyquist (4.571 MHz)
        # a mask 15 dB under the band at 4.0 MHz, 25 dB at 4.4: the louder lower bin (-20 dB at 4.205 MHz) misses it by about 0.1 dB
        m = r.mask_margin(((4.0e6, -15.0), (4.4e6, -25.0)), HB)
        fb = np.abs(f[int(np.argmin(np.abs(f + (HB + 400e3))))])
        assert m == pytest.approx(-15.0 - 10.0 * (fb - 4.0e6) / 0.4e6 + 20.0, abs=1e-9)


def test_the_helpers_equal_the_models(g):
    rng = np.random.RandomState(4)
    f, psd, hist = _brick()
    psd = psd * rng.uniform(0.5, 2.0, len(psd))
    a, b = _both(g, psd, hist)
    assert np.array_equal(a.freqs(), b.freqs()) and np.array_equal(a.freqs(8e6), b.freqs(8e6))
    assert a.mean_power == b.mean_power == 1.5 and a.enbw == b.enbw
    assert a.band_power(-1e6, 2e6) == pytest.approx(b.band_power(-1e6, 2e6), rel=1e-14)
    for frac in (0.5, 0.9, 0.99, 0.9999):
        assert a.occupied_bandwidth(frac) == b.occupied_bandwidth(frac)
    assert a.shoulder_db(HB) == pytest.approx(b.shoulder_db(HB), rel=1e-14)
    assert a.shoulder_db(HB, 100e3, 200e3) == pytest.approx(b.shoulder_db(HB, 100e3, 200e3), rel=1e-14)
    (la, pa), (lb, pb) = a.ccdf(), b.ccdf()
    assert np.array_equal(la, lb) and np.allclose(pa, pb, rtol=1e-14, atol=0) and pa[1015] == 1.0 and pa[1016] == 0.1 and pa[1040] == 0.0
    for prob in (None, 0.5, 0.1, 0.05, 0.01, 0.001):
        assert a.papr_db(prob) == pytest.approx(b.papr_db(prob), rel=1e-13)
    pts = ((3.9e6, -10.0), (4.2e6, -20.0), (4.5e6, -40.0))
    assert a.mask_margin(pts, HB) == pytest.approx(b.mask_margin(pts, HB), rel=1e-13)
    for kind in (0, 1, 2):
        assert np.array_equal(g.spectrum_window(512, kind), sr.window(512, kind))


@pytest.mark.parametrize("n,N,hop,S", [(63, 64, 32, 0), (64, 64, 32, 1), (95, 64, 32, 1), (96, 64, 32, 2), (1000, 64, 24, 40), (1000, 128, 128, 7), (1000, 128, 16, 55)])
def test_the_statistics_cover_the_first_hop_samples_of_every_segment(n, N, hop, S):
    x = np.full(n, 1 + 0j, np.complex64)
    x[S * hop:] = 4.0                                      # behind the counted range: must not be seen
    r = sr.welch(x, N, hop, sr.RECT)
    assert (r.segments, r.samples_pushed, r.samples_counted) == (S, n, S * hop) and sr.segments(n, N, hop) == S
    assert int(r.hist.sum()) == S * hop == int(r.hist[1016]) and r.sum_power == S * hop
    assert float(r.peak_power) == (1.0 if S else 0.0)


# ------------------------------------------------------------------ the experiment behind the block: an amplifier's spectral regrowth on the project's own signal
@pytest.fixture(scope="module")
def ofdm(po):
    c = po.cfg(po.QAM16, po.C1_2, po.T2k)
    iq = po.tx(c, po.stream_ts(c, 0, 1, 7))
    sym = c.N + c.cp
    return iq[20 * sym:220 * sym]


def test_the_shoulder_falls_with_the_amplifiers_back_off(ofdm):
    ref_power = float(np.mean(np.abs(ofdm.astype(np.complex128)) ** 2))
    shoulders = []
    for ibo in (None, 12.0, 9.0, 6.0, 3.0):
        y = ofdm if ibo is None else rr.pa(ofdm, rr.saturation(ibo, ref_power), 2.0).astype(np.complex64)
        r = sr.welch(y, 1024, 512, sr.HANN)
        assert r.segments == 824
        shoulders.append(r.shoulder_db(HB))
        assert r.psd.sum() == pytest.approx(r.mean_power, rel=2e-3)
    print("\nshoulders (lower, upper) without an amplifier and at 12, 9, 6, 3 dB of back-off:", [(round(a, 1), round(b, 1)) for a, b in shoulders])
    for side in (0, 1):
        s = [v[side] for v in shoulders]
        assert all(s[i] > s[i + 1] for i in range(4))
        assert all(s[i] - s[i + 1] > 1.0 for i in (1, 2, 3))
        assert abs(s[0] - (31.0, 30.5)[side]) <= 0.3 and abs(s[4] - (17.8, 17.6)[side]) <= 0.3      # the figures of the float64 session behind this block
    r0 = sr.welch(ofdm, 1024, 512, sr.HANN)
    assert r0.occupied_bandwidth(0.99) <= 1705 * FS / 2048
