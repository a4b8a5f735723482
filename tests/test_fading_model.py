"""The fading block's model (tests/fadingref.py) against what it claims: a deterministic counter-based table, Clarke's spectrum (arcsine-distributed
frequencies, J0 autocorrelation), the chord bound of the piecewise-linear gain, unit mean power of the scatter, and COST 207 TU6."""
import math

import numpy as np
import pytest

import chanref
import fadingref as fr

P24 = tuple((i, 0.0, 1.0) for i in range(24))


def test_the_table_is_deterministic_and_depends_on_seed_and_path():
    p = fr.params(P24, 1e-5, 16, seed=7)
    inc, ph = fr.table(p)
    assert (inc, ph) == fr.table(fr.params(P24, 1e-5, 16, seed=7))
    inc2, ph2 = fr.table(fr.params(P24, 1e-5, 16, seed=8))
    assert all(a != b for a, b in zip(sum(ph, []), sum(ph2, []))) and inc != inc2
    rows = [tuple(r) for r in ph]
    assert len(set(rows)) == 24 and len(set(sum(ph, []))) == 24 * 16          # other paths, other words
    assert len(set(tuple(r) for r in inc)) == 24
    # the high half of the seed is part of the key
    assert fr.table(fr.params(P24, 1e-5, 16, seed=7 + 2 ** 32))[1] != ph


def test_the_tagged_counter_is_not_the_noise_generators():
    for seed in (0, 7, 2 ** 63 + 5):
        key = (seed & 0xffffffff, seed >> 32)
        for m, i in ((0, 0), (3, 0), (5, 2), (31, 23)):
            tagged = chanref.philox4x32((m, i, 0, fr.TAG), key).reshape(4)
            noise = chanref.philox4x32((m, i, 0, 0), key).reshape(4)           # the block of pair P = m + 2^32 i of the noise
            assert not (tagged == noise).any()


@pytest.mark.parametrize("M", [1, 7, 16, 32])
@pytest.mark.parametrize("doppler", [0.0, 1e-5, fr.MAX_DOPPLER])
def test_every_frequency_is_within_the_doppler(M, doppler):
    f = fr.freqs(fr.params(P24, doppler, M, seed=11))
    assert f.shape == (24, M) and (np.abs(f) <= doppler).all()
    if doppler == 0.0:
        assert (f == 0).all()


@pytest.mark.parametrize("M", [8, 16, 32])
def test_frequencies_follow_the_arcsine_law(M):
    doppler = 1e-4
    v = np.sort((fr.freqs(fr.params(P24, doppler, M, seed=3)) / doppler).reshape(-1))
    cdf = 1.0 - np.arccos(np.clip(v, -1, 1)) / np.pi
    n = len(v)
    hi = np.arange(1, n + 1) / n - cdf                 # the empirical distribution just behind and just in front of every jump: its extremes are there
    lo = cdf - np.arange(0, n) / n
    assert max(hi.max(), lo.max()) <= 2.0 / M


def _j0(x):
    th = (np.arange(4096) + 0.5) * (np.pi / 4096)
    return np.cos(np.outer(x, np.sin(th))).mean(axis=1)


def test_ensemble_autocorrelation_is_j0():
    doppler = 1e-4
    f = np.concatenate([fr.freqs(fr.params(P24, doppler, 16, seed=s)).reshape(-1) for s in range(1, 9)])
    assert len(f) == 8 * 24 * 16
    dt = np.linspace(0.0, 2.0, 201)                    # doppler tau
    r = np.exp(2j * np.pi * np.outer(dt, f / doppler)).mean(axis=1)
    err = np.abs(r - _j0(2 * np.pi * dt)).max()
    print("largest distance from J0:", err)
    assert err <= 0.05


@pytest.mark.parametrize("doppler", [200.0 / (64e6 / 7), fr.MAX_DOPPLER])
@pytest.mark.parametrize("first", [0, 2 ** 40 + 3])
def test_gains_stay_within_the_chord_bound(doppler, first):
    p = fr.params(((0, 0.25 - 0.5j, 1.0), (5, 0.0, 0.5)), doppler, 16, seed=5)
    n = 64 * 40 + 7
    d = np.abs(fr.gains(p, first, n) - fr.exact_gains(p, first, n))
    for i in range(2):
        b = fr.chord_bound(p, i)
        print(doppler, first, i, "distance", d[i].max(), "bound", b)
        assert d[i].max() <= b
        if doppler == fr.MAX_DOPPLER:
            assert d[i].max() >= 0.1 * b
    k = first + np.arange(n)
    at = (k & 63) == 0
    assert d[:, at].max() < 1e-12                      # a knot is the sum itself


def test_mean_power_of_the_scatter_is_sigma_squared():
    sigma = 0.75
    acc = []
    for seed in range(64):
        G = fr.knots(fr.params(tuple((0, 0.0, sigma) for _ in range(24)), 1e-4, 16, seed=1000 + seed), 12345, 1)
        acc.append(np.abs(G[:, 0]) ** 2)
    mean = np.concatenate(acc).mean()
    print("mean |G|^2 / sigma^2:", mean / sigma ** 2)
    assert abs(mean / sigma ** 2 - 1.0) <= 0.10


def test_tu6():
    paths, dop = fr.tu6(100.0)
    assert tuple(d for d, _, _ in paths) == (0, 2, 5, 15, 21, 46)
    assert dop == 100.0 / (64e6 / 7)
    assert abs(sum(abs(l) ** 2 + s * s for _, l, s in paths) - 1.0) < 1e-12
    assert all(l == 0 for _, l, _ in paths)
    rel = [s * s for _, _, s in paths]
    want = [10 ** (d / 10) for d in fr.TU6_POWERS_DB]
    assert np.allclose(np.array(rel) / rel[1], np.array(want) / want[1], rtol=1e-12)
    rp, _ = fr.tu6(100.0, rice_k_db=10.0)
    assert tuple(d for d, _, _ in rp) == (0, 2, 5, 15, 21, 46)
    tot = sum(abs(l) ** 2 + s * s for _, l, s in rp)
    assert abs(tot - 1.0) < 1e-12
    assert abs(abs(rp[0][1]) ** 2 / tot - 10.0 / 11.0) < 1e-12 and all(l == 0 for _, l, _ in rp[1:])
    assert np.allclose([s * s for _, _, s in rp], np.array(rel) / 11.0, rtol=1e-12)


def test_fading_is_the_sum_over_the_paths():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(300) + 1j * rng.standard_normal(300)
    p = fr.params(((0, 1.0, 0.0), (3, 0.0, 0.5), (3, 0.25j, 0.0)), 1e-4, 4, seed=2)
    g = fr.gains(p, 77, 300)
    y = fr.fading(x, p, 77)
    n = 200
    assert abs(y[n] - (g[0, n] * x[n] + g[1, n] * x[n - 3] + g[2, n] * x[n - 3])) < 1e-12
    assert abs(y[1] - g[0, 1] * x[1]) < 1e-15                                  # x is 0 in front of the stream
    assert np.array_equal(fr.fading(x, fr.params(((0, 1.0, 0.0),)), 5), x)
