"""CPU-side checks of the RF front-end block's C ABI (include/dvbt_hip.h, dvbt_rf_*): exported, laid out as the binding says, every parameter checked before
the device is asked for, no CPU fallback, and the host's tone table of a phase-noise mask equal to the model's (tests/rfref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rfref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_SYMBOLS = ("dvbt_rf_phase_noise_tones", "dvbt_rf_create", "dvbt_rf_run", "dvbt_rf_run_device", "dvbt_rf_reset", "dvbt_rf_destroy")
FIELDS = ("sat_amplitude", "smoothness", "n_tones", "tone_inc", "tone_phase", "tone_amp", "mu_re", "mu_im", "nu_re", "nu_im", "dc_re", "dc_im",
          "first_sample", "device")
MASK_FIELDS = ("n_points", "offset_hz", "dbc_hz", "sample_rate")
FAR = 2 ** 40 + 3
NAN, INF = float("nan"), float("inf")
MASK_10 = ((100.0, -60.0), (1e3, -70.0), (1e4, -80.0), (1e5, -100.0), (1e6, -120.0))
MASK_OTHER = ((250.0, -55.0), (3e3, -81.0), (7e4, -96.0), (2.5e6, -131.0))
TONES3 = ((1 << 40, 2 ** 64 - 1, 12345), (0, 1 << 63, 2 ** 64 - 1), (0.5, 0.0, 1.0))


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _create(g, p):
    L = g.lib()
    L.dvbt_rf_create.argtypes = [C.POINTER(g.RfParams), C.POINTER(C.c_void_p)]
    L.dvbt_rf_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_rf_create(C.byref(p), C.byref(h))
    if h.value:
        L.dvbt_rf_destroy(h)
    return r, bool(h.value)


def _mask(g, points, sample_rate=rr.SAMPLE_RATE):
    mk = g.RfMask()
    mk.n_points, mk.sample_rate = len(points), sample_rate
    for k, (f, d) in enumerate(points[:8]):
        mk.offset_hz[k], mk.dbc_hz[k] = f, d
    return mk


def _tones(g, mk, n_tones=32, seed=0):
    """(the C function's return value, whether the output arrays are untouched)"""
    L = g.lib()
    L.dvbt_rf_phase_noise_tones.argtypes = [C.POINTER(g.RfMask), C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    inc, ph, amp = (C.c_uint64 * 40)(), (C.c_uint64 * 40)(), (C.c_float * 40)()
    for i in range(40):
        inc[i] = ph[i] = 0xdeadbeef
        amp[i] = -7.0
    r = L.dvbt_rf_phase_noise_tones(C.byref(mk), n_tones, seed, inc, ph, amp)
    return r, all(v == 0xdeadbeef for v in inc) and all(v == 0xdeadbeef for v in ph) and all(v == -7.0 for v in amp)


def test_every_rf_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in RF_SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    assert (g.RF_MAX_TONES, g.RF_MAX_MASK_POINTS) == (32, 8) == (rr.MAX_TONES, rr.MAX_MASK_POINTS)


def test_rf_structs_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    n = len(FIELDS) + 1 + len(MASK_FIELDS) + 1
    fmt = " ".join(["%zu"] * n) + " %d %d"
    offs = ", ".join(f"offsetof(dvbt_rf_params, {f})" for f in FIELDS)
    moffs = ", ".join(f"offsetof(dvbt_rf_mask, {f})" for f in MASK_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dvbt_rf_params), {offs}, sizeof(dvbt_rf_mask), {moffs}, DVBT_RF_MAX_TONES, '
                   'DVBT_RF_MAX_MASK_POINTS); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, M = g.RfParams, g.RfMask
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] + [C.sizeof(M)] + [getattr(M, f).offset for f in MASK_FIELDS]
    assert got[:-2] == want
    assert want == [696, 0, 4, 8, 16, 272, 528, 656, 660, 664, 668, 672, 676, 680, 688, 144, 0, 8, 72, 136]
    assert got[-2:] == [32, 8]


def test_rf_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _create(g, g.RfParams()) == (-2, False)                             # a zeroed struct is a good one: the identity
    assert _create(g, g.RfParams.of()) == (-2, False)
    mu, nu = g.RfFrontend.iq_imbalance(0.5, 3.0)
    tones = g.phase_noise_tones(MASK_10, 32, seed=2 ** 64 - 1)
    assert _create(g, g.RfParams.of(0.7, 16.0, tones, mu, nu, 0.01 - 0.02j, FAR)) == (-2, False)
    assert _create(g, g.RfParams.of(1e-30, 0.5, TONES3)) == (-2, False)
    assert _create(g, g.RfParams.of(tones=((1, 2), (3, 4), (3.0, 0.1415)))) == (-2, False)
    with pytest.raises(g.DvbtError) as e:
        g.RfFrontend()
    assert "no CPU fallback" in str(e.value)


BAD = {
    "negative sat_amplitude": dict(sat_amplitude=-1.0),
    "nan sat_amplitude": dict(sat_amplitude=NAN),
    "infinite sat_amplitude": dict(sat_amplitude=INF),
    "smoothness below 0.5": dict(sat_amplitude=1.0, smoothness=0.4999),
    "smoothness above 16": dict(sat_amplitude=1.0, smoothness=16.001),
    "negative smoothness": dict(smoothness=-2.0),
    "nan smoothness": dict(smoothness=NAN),
    "negative amplitude": dict(tones=((1, 2), (3, 4), (0.1, -0.1))),
    "nan amplitude": dict(tones=((1, 2), (3, 4), (NAN, 0.1))),
    "infinite amplitude": dict(tones=((1,), (3,), (INF,))),
    "amplitudes above pi": dict(tones=((1, 2, 3), (4, 5, 6), (1.5, 1.5, 0.1416))),
    "nan mu": dict(mu=complex(NAN, 0.0)),
    "infinite mu": dict(mu=complex(1.0, INF)),
    "nan nu": dict(nu=complex(0.0, NAN)),
    "infinite nu": dict(nu=complex(-INF, 0.0)),
    "nan dc": dict(dc=complex(NAN, 0.0)),
    "infinite dc": dict(dc=complex(0.0, INF)),
    "negative first_sample": dict(first_sample=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, g.RfParams.of(**BAD[name])) == (-1, False), name
    assert g.lib().dvbt_last_error()
    with pytest.raises(g.DvbtError):
        g.RfFrontend(**BAD[name])


@pytest.mark.parametrize("n_tones", [33, -1])
def test_a_bad_tone_count_is_refused(g, n_tones):
    p = g.RfParams.of(tones=TONES3)
    p.n_tones = n_tones
    assert _create(g, p) == (-1, False)
    with pytest.raises(ValueError):
        g.RfParams.of(tones=(list(range(33)), list(range(33)), [0.01] * 33))


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_rf_create.argtypes = [C.POINTER(g.RfParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_rf_create(None, C.byref(h)) == -1
    assert L.dvbt_rf_create(C.byref(g.RfParams()), None) == -1
    L.dvbt_rf_phase_noise_tones.argtypes = [C.POINTER(g.RfMask), C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    w, a, mk = (C.c_uint64 * 32)(), (C.c_float * 32)(), _mask(g, MASK_10)
    assert L.dvbt_rf_phase_noise_tones(None, 8, 0, w, w, a) == -1
    assert L.dvbt_rf_phase_noise_tones(C.byref(mk), 8, 0, None, w, a) == -1
    assert L.dvbt_rf_phase_noise_tones(C.byref(mk), 8, 0, w, None, a) == -1
    assert L.dvbt_rf_phase_noise_tones(C.byref(mk), 8, 0, w, w, None) == -1
    assert not any(w) and not any(a)
    L.dvbt_rf_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.dvbt_rf_run(None, None, 0, None) == -1
    L.dvbt_rf_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert L.dvbt_rf_run_device(None, None, 0, None, None) == -1
    L.dvbt_rf_reset.argtypes = [C.c_void_p]
    assert L.dvbt_rf_reset(None) == -1
    L.dvbt_rf_destroy.argtypes = [C.c_void_p]
    L.dvbt_rf_destroy(None)


BAD_MASKS = {
    "one point": dict(points=MASK_10[:1]),
    "nine points": dict(points=tuple((100.0 * 2 ** k, -60.0 - k) for k in range(9))),
    "offsets not ascending": dict(points=((100.0, -60.0), (1e4, -80.0), (1e3, -70.0))),
    "equal offsets": dict(points=((100.0, -60.0), (100.0, -70.0))),
    "an offset of 0": dict(points=((0.0, -60.0), (1e3, -70.0))),
    "a negative offset": dict(points=((-5.0, -60.0), (1e3, -70.0))),
    "last offset above half the sample rate": dict(points=((100.0, -60.0), (rr.SAMPLE_RATE / 2 * (1 + 1e-12), -120.0))),
    "a nan level": dict(points=((100.0, NAN), (1e3, -70.0))),
    "an infinite level": dict(points=((100.0, -60.0), (1e3, -INF))),
    "a nan offset": dict(points=((100.0, -60.0), (NAN, -70.0))),
    "a sample rate of 0": dict(points=MASK_10[:2], sample_rate=0.0),
    "a nan sample rate": dict(points=MASK_10[:2], sample_rate=NAN),
    "no tones": dict(points=MASK_10, n_tones=0),
    "33 tones": dict(points=MASK_10, n_tones=33),
    "negative tones": dict(points=MASK_10, n_tones=-1),
}


@pytest.mark.parametrize("name", sorted(BAD_MASKS))
def test_bad_masks_are_refused_and_nothing_is_written(g, name):
    b = BAD_MASKS[name]
    mk = _mask(g, b["points"], b.get("sample_rate", rr.SAMPLE_RATE))
    assert _tones(g, mk, b.get("n_tones", 32)) == (-1, True), name
    assert g.lib().dvbt_last_error()
    with pytest.raises((g.DvbtError, ValueError)):
        g.phase_noise_tones(b["points"], b.get("n_tones", 32), 0, b.get("sample_rate", rr.SAMPLE_RATE))


def test_the_largest_mask_is_taken(g):
    pts = tuple((100.0 * 4 ** k, -60.0 - 7 * k) for k in range(7)) + ((rr.SAMPLE_RATE / 2, -140.0),)
    assert _tones(g, _mask(g, pts), 32)[0] == 0
    inc, _, _ = g.phase_noise_tones(pts, 32, 1)
    assert int(inc.max()) <= 2 ** 63


@pytest.mark.parametrize("seed", [0, 0xfedcba9876543210])
@pytest.mark.parametrize("mask", [MASK_10, MASK_OTHER], ids=["with_-10dB_per_decade", "without"])
@pytest.mark.parametrize("M", [1, 8, 32])
def test_the_hosts_table_equals_the_models(g, M, mask, seed):
    inc, ph, amp = g.phase_noise_tones(mask, M, seed)
    ri, rp, ra = rr.tones(mask, M, seed)
    assert inc.shape == ph.shape == amp.shape == (M,) and amp.dtype == np.float32
    assert [int(v) for v in ph] == rp                                          # integers: word for word
    f = rr.tone_freqs(mask, M, seed)
    for m in range(M):                                                         # two libraries' exp and log, each good to an ulp, magnified by ln rho <= 14
        assert abs(int(inc[m]) - ri[m]) <= 1e-12 * f[m] / rr.SAMPLE_RATE * 2.0 ** 64 + 1, m
    assert np.abs(amp.astype(np.float64) / ra.astype(np.float64) - 1.0).max() <= 1e-6
    other = g.phase_noise_tones(mask, M, seed + 1)
    assert (other[1] != ph).all() and np.array_equal(other[2], amp)


def test_the_helpers(g):
    assert g.RfFrontend.saturation(6.0, 0.25) == pytest.approx(rr.saturation(6.0, 0.25), rel=1e-15)
    assert g.RfFrontend.saturation(0.0, 4.0) == 2.0
    mu, nu = g.RfFrontend.iq_imbalance(0.5, 3.0)
    rmu, rnu = rr.iq_imbalance(0.5, 3.0)
    assert abs(mu - rmu) <= 1e-15 and abs(nu - rnu) <= 1e-15
    assert abs(rr.irr_db(mu, nu) - 28.2) <= 0.05
    assert g.RfFrontend.iq_imbalance(0.0, 0.0) == (1.0, 0.0)
