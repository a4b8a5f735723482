"""The constellation analyser's definitions (include/dvbt_hip.h) as tests/constref.py models them, and the host figures of gr_dvbt_amd.ConstellationReading
on the model's sums.  numpy only: nothing here needs a GPU or the built library.

Where a figure is compared with a known one the bound derives from the quantisation: a cell's error is rounded to 2^-12 d, i.e. moved by at most a half step
2^-13 d per axis, against levels of at least d."""
import numpy as np
import pytest

import constref as cr
import qualref

import gr_dvbt_amd as g

GRID_IDS = [f"c{c}h{h}" for c, h in cr.GRIDS]


def _one(x, c, h):
    """the axis record of a single float"""
    r = cr.axis(np.array([x], np.float32), c, h)
    return {k: v[0] for k, v in r.items()}


@pytest.mark.parametrize("c,h", cr.GRIDS, ids=GRID_IDS)
def test_ideal_points_have_no_error(c, h):
    L, H, alpha, S, inv_d = cr.grid(c, h)
    pts = cr.ideal_cells(c, h)
    assert len(pts) == L * L
    r = cr.analyse(pts.reshape(1, -1), c, h)
    assert (r.points["n"] == 1).all(), "every point is hit once, in the order p = row L + col"
    for f in ("sum_re", "sum_im", "sum_re_im", "sum_re2", "sum_im2"):
        assert not r.points[f].any(), f
    assert not r.carriers["error"].any() and (r.nonfinite, r.clipped, r.cells) == (0, 0, L * L)
    want = r.ideal
    assert np.array_equal(r.carriers["signal"], (want ** 2).sum(axis=1).astype(np.int64))
    assert (r.levels, r.alpha, r.span) == (L, alpha, S) == g.constellation_grid(c, h)
    assert np.allclose(want[:, 0] + 1j * want[:, 1], pts * np.float64(inv_d), atol=1e-5)
    assert np.isinf(r.mer_db) and r.ste() == (0.0, 0.0)


@pytest.mark.parametrize("c,h", cr.GRIDS, ids=GRID_IDS)
def test_cells_on_the_edges_go_where_the_definition_says(c, h):
    L, H, alpha, S, inv_d = cr.grid(c, h)
    d = 1.0 / np.float64(inv_d)
    # decision boundaries: t = j exactly belongs to level j, the float below it to level j - 1
    for j in range(1, H):
        b = np.float32((alpha - 1 + 2 * j) * d)
        for x in (b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(100))):
            t = np.float32((np.float32(x * inv_d) - np.float32(alpha - 1)) * np.float32(0.5))
            want = min(int(t), H - 1) if t >= 1 else 0
            got = _one(x, c, h)
            assert got["j"] == want and got["level"] == alpha + 2 * want and got["idx"] == H + want
            assert _one(-x, c, h)["idx"] == H - 1 - want and _one(-x, c, h)["q"] == -got["q"]
    # below the lowest and beyond the highest level: the outer points own the rest of the axis
    assert _one(0.25 * d, c, h)["j"] == 0 and _one(40.0 * d, c, h)["j"] == H - 1
    # +-0.0: the sign bit decides the side, the error is the whole level
    zp, zn = _one(0.0, c, h), _one(-0.0, c, h)
    assert (zp["idx"], zp["q"], zp["bin"]) == (H, -4096 * alpha, cr.G // 2)
    assert (zn["idx"], zn["q"], zn["bin"]) == (H - 1, 4096 * alpha, cr.G // 2), "e = -0.0 floors to -0.0: bin G / 2"
    # denormals: finite, next to nothing
    for x, idx, b in ((1e-40, H, cr.G // 2), (-1e-40, H - 1, cr.G // 2 - 1), (1.4e-45, H, cr.G // 2)):
        r = _one(x, c, h)
        assert not r["nonfinite"] and (r["idx"], abs(r["q"]), r["bin"], r["clipped"]) == (idx, 4096 * alpha, b, False)
    # 1e30: clipped, clamped, the edge bin; 3e38 inv_d overflows to inf and goes the same way
    for x in (1e30, 3e38):
        r, m = _one(x, c, h), _one(-x, c, h)
        assert (r["q"], r["clipped"], r["bin"], r["idx"], r["nonfinite"]) == (32767, True, cr.G - 1, L - 1, False)
        assert (m["q"], m["clipped"], m["bin"], m["idx"]) == (-32767, True, 0, 0)
    # the clip's threshold: |r| = 32767 is not clipped, 32768 is
    u_edge = (alpha + 2 * (H - 1)) + 32767.0 / 4096.0
    assert not _one(np.float32(u_edge * d * (1 - 1e-6)), c, h)["clipped"] and _one(np.float32((u_edge + 4.0 / 4096.0) * d), c, h)["clipped"]
    # histogram bin edges: u = k 2 S / G opens bin G / 2 + k
    k = np.float32(cr.G // (2 * S))
    for e in (-cr.G // 2, -1, 1, 3, cr.G // 2 - 1):
        b = np.float32(e * 2.0 * S / cr.G * d)
        for x in (b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(100) * np.sign(b))):
            u = np.float32(abs(x) * inv_d)
            want = int(np.clip(np.floor((-u if x < 0 else u) * k), -cr.G // 2, cr.G // 2 - 1)) + cr.G // 2
            assert _one(x, c, h)["bin"] == want
    assert _one(np.float32(S * d * 1.001), c, h)["bin"] == cr.G - 1 and _one(np.float32(-S * d * 1.001), c, h)["bin"] == 0
    # non-finite on either axis: counted, nothing else
    cells = np.array([[np.inf + 0j, complex(0, np.nan), complex(-np.inf, 1), complex(np.nan, np.nan), cr.ideal_cells(c, h)[0]]], np.complex64)
    r = cr.analyse(cells, c, h)
    assert (r.nonfinite, r.cells, int(r.hist.sum()), int(r.points["n"].sum())) == (4, 5, 1, 1)
    assert r.carriers["n"].tolist() == [0, 0, 0, 0, 1]
    # the special cells as a whole: the sums account for every finite cell once
    sp = cr.special_cells(c, h)
    r = cr.analyse(sp.reshape(1, -1), c, h)
    assert r.nonfinite > 0 and r.clipped > 0
    assert int(r.hist.sum()) == int(r.points["n"].sum()) == int(r.carriers["n"].sum()) == r.cells - r.nonfinite
    assert int(r.points["sum_re2"].sum() + r.points["sum_im2"].sum()) == int(r.carriers["error"].sum())


def test_the_model_sees_an_fma_contraction():
    """the GPU tests compare with the model for equality; this shows that they would see a contracted a inv_d - level"""
    total = 0
    for c, h in cr.GRIDS:
        cells = cr.stream(c, h, 33, 257)
        a, b = cr.bits_of(cr.analyse(cells, c, h)), cr.bits_of(cr.analyse(cells, c, h, contract=True))
        x, y = cr.axis(cells.real.reshape(-1), c, h), cr.axis(cells.real.reshape(-1), c, h, contract=True)
        differ = int((x["q"] != y["q"]).sum())
        total += differ
        print(f"grid {c},{h}: {differ} of {cells.size} real parts quantise differently when contracted")
        assert differ >= 1 and a != b, (c, h)
    assert total >= 7


def _noise_free(c, h, A, b, reps=3):
    """every point `reps` times, mapped by A x + b (grid units), as cells"""
    L, H, alpha, S, inv_d = cr.grid(c, h)
    ideal = cr.analyse(cr.ideal_cells(c, h).reshape(1, -1), c, h).ideal
    z = ideal @ np.asarray(A).T + np.asarray(b)
    cells = ((z[:, 0] + 1j * z[:, 1]) / np.float64(inv_d)).astype(np.complex64)
    return np.tile(cells, reps).reshape(reps, -1), ideal


@pytest.mark.parametrize("c,h", [(1, 0), (2, 0), (2, 2), (1, 3)], ids=["qam16", "qam64", "qam64a2", "qam16a4"])
def test_the_fit_returns_a_known_map(c, h):
    th, gi, gq = np.radians(1.5), 1.02, 0.99                               # Q's axis leans by 1.5 degrees, I is 3 % longer than Q
    A = np.array([[gi, -gq * np.sin(th)], [0.0, gq * np.cos(th)]])
    b = np.array([0.03, -0.02])
    cells, ideal = _noise_free(c, h, A, b)
    r = cr.analyse(cells, c, h)
    assert (r.points["n"] == 3).all(), "the map is small enough to keep every cell at its own point"
    A_got, b_got = r.fit()
    # every mean is off by at most a half step 2^-13 d per axis; a least-squares fit over points of at least d does not amplify that
    assert np.abs(A_got - A).max() <= 1e-3 and np.abs(b_got - b).max() <= 1e-3 * np.abs(b).max() + 2.0 ** -13
    assert abs(r.amplitude_imbalance_pct - (gi / gq - 1.0) * 100.0) <= 1e-3 * 100.0
    assert abs(r.quadrature_error_deg - (-1.5)) <= np.degrees(2e-3), "90 degrees minus the angle between the columns: the lean, signed"
    sup = 10.0 * np.log10((ideal ** 2).sum(axis=1).mean() / (b @ b))
    assert abs(r.carrier_suppression_db - sup) <= 20.0 * np.log10(1.0 + 2.0 ** -13 * np.sqrt(2.0) / np.hypot(*b)) + 1e-3
    d = ideal @ A.T + b - ideal
    s = np.hypot(d[:, 0], d[:, 1]) / np.sqrt((ideal ** 2).sum(axis=1).mean())
    stem, sted = r.ste()
    assert abs(stem - s.mean()) <= 1e-3 * s.mean() + 1e-4 and abs(sted - s.std()) <= 1e-3 * s.std() + 1e-4


def test_empty_inputs_read_as_nan():
    r = cr.analyse(np.zeros((0, 7), np.complex64), 2, 0)
    assert r.cells == 0 and not r.hist.any()
    for v in (r.mer_db, r.carrier_suppression_db, r.amplitude_imbalance_pct, r.quadrature_error_deg, r.phase_jitter_deg, *r.ste()):
        assert np.isnan(v)
    assert np.isnan(r.mer_per_carrier_db).all() and len(r.mer_per_carrier_db) == 7
    A, b = r.fit()
    assert np.isnan(A).all() and np.isnan(b).all()


@pytest.mark.parametrize("c,h", [(0, 0), (2, 0), (2, 3)], ids=["qpsk", "qam64", "qam64a4"])
def test_a_known_tangential_jitter_reads_back(c, h):
    """the four corners moved along their tangents by rho tan(phi_k) for an enumerated, symmetric set of angles, plus the same enumerated offsets along both
    axes (an isotropic cloud, which the radial variance takes out again): the expected figure is the set's own rms"""
    L, H, alpha, S, inv_d = cr.grid(c, h)
    ideal = cr.analyse(cr.ideal_cells(c, h).reshape(1, -1), c, h).ideal
    corners = ideal[[0, L - 1, L * (L - 1), L * L - 1]]
    phis = np.radians(np.linspace(-2.0, 2.0, 41))
    iso = np.array([(0.0, 0.0), (0.05, 0.0), (-0.05, 0.0), (0.0, 0.05), (0.0, -0.05)])
    cells = []
    for x, y in corners:
        rho = np.hypot(x, y)
        tan_v = np.array([-y, x]) / rho
        for p in phis:
            for o in iso:
                z = np.array([x, y]) + rho * np.tan(p) * tan_v + o
                cells.append(complex(*z))
    cells = (np.array(cells) / np.float64(inv_d)).astype(np.complex64).reshape(1, -1)
    r = cr.analyse(cells, c, h)
    assert int(r.points["n"][[0, L - 1, L * (L - 1), L * L - 1]].sum()) == cells.size
    want = np.degrees(np.sqrt(np.mean(np.tan(phis) ** 2)))
    # the quantisation moves a cell by at most 2^-13 sqrt(2) d against displacements of rho tan(phi): 1e-3 relative covers it
    assert abs(r.phase_jitter_deg - want) <= 1e-3 * want, (r.phase_jitter_deg, want)
    clean = cr.analyse(np.tile(cr.ideal_cells(c, h), 4).reshape(4, -1), c, h)
    assert clean.phase_jitter_deg == 0.0


def test_mer_from_the_sums_is_the_quality_models():
    """20 dB on QAM64: the relative change of the error sum by the quantisation is at most 2 eps / sigma, eps = sqrt(2) 2^-13 d and sigma = 0.65 d, i.e.
    5e-4 or 0.002 dB; the threshold rule and the nearest point agree except on ties.  0.01 dB is asked."""
    for c, m in ((0, 2), (1, 4), (2, 6)):
        cells = cr.stream(c, 0, 64, 1512, seed=5, snr_db=20.0, specials=False)
        r = cr.analyse(cells, c, 0)
        n, sig, err = qualref.mer(cells, m)
        assert n == r.cells and r.nonfinite == 0
        assert abs(r.mer_db - qualref.mer_db(sig, err)) <= 0.01, (c, r.mer_db, qualref.mer_db(sig, err))
        per = r.mer_per_carrier_db
        assert per.shape == (1512,) and np.isfinite(per).all()
