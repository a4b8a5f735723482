"""CPU-side checks of the signal scanner's C ABI (include/dvbt_hip.h, dvbt_scan_*): exported, laid out as the binding says, every parameter checked before
the device is asked for, no CPU fallback for the handle -- and dvbt_scan_evaluate, which is host arithmetic, against tests/scanref.py's evaluation."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import scanref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvbt_scan_create", "dvbt_scan_push", "dvbt_scan_push_device", "dvbt_scan_read", "dvbt_scan_accumulators", "dvbt_scan_evaluate",
           "dvbt_scan_reset", "dvbt_scan_destroy")
P_FIELDS = ("device", "rho_min", "ratio_min")
R_FIELDS = ("detected", "mode", "guard", "symbol_start", "samples_pushed", "nonfinite", "symbols", "rho", "cfo")


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _create(g, rho_min=0.0, ratio_min=0.0, device=0):
    L = g.lib()
    L.dvbt_scan_create.argtypes = [C.POINTER(g.ScanParams), C.POINTER(C.c_void_p)]
    L.dvbt_scan_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_scan_create(C.byref(g.ScanParams(device, rho_min, ratio_min)), C.byref(h))
    if h.value:
        L.dvbt_scan_destroy(h)
    return r, bool(h.value)


def test_every_scan_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    assert (g.SCAN_GROUP, g.SCAN_MIN_SAMPLES, g.SCAN_HYPOTHESES) == (scanref.GROUP, scanref.MIN_SAMPLES, scanref.HYPS) == (16, 90112, 8)
    assert [g.scan_dims(h) for h in range(8)] == [scanref.dims(h) for h in range(8)]
    for name in ("Scanner", "ScanReading", "ScanParams", "ScanResult", "scan_evaluate"):
        assert hasattr(g, name)


def test_scan_structs_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    n = len(P_FIELDS) + 1 + len(R_FIELDS) + 1
    fmt = " ".join(["%zu"] * n) + " %d %d %d"
    poffs = ", ".join(f"offsetof(dvbt_scan_params, {f})" for f in P_FIELDS)
    roffs = ", ".join(f"offsetof(dvbt_scan_result, {f})" for f in R_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dvbt_scan_params), {poffs}, sizeof(dvbt_scan_result), {roffs}, '
                   'DVBT_SCAN_HYPOTHESES, DVBT_SCAN_GROUP, DVBT_SCAN_MIN_SAMPLES); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, R = g.ScanParams, g.ScanResult
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in P_FIELDS] + [C.sizeof(R)] + [getattr(R, f).offset for f in R_FIELDS]
    assert got[:-3] == want
    assert want == [24, 0, 8, 16, 256, 0, 4, 8, 12, 48, 56, 64, 128, 192]
    assert got[-3:] == [8, 16, 90112]


def test_scan_create_has_no_cpu_fallback(g):
    want = (0, True) if g.device_count() > 0 else (-2, False)
    for rho_min, ratio_min in ((0.0, 0.0), (0.1, 1.5), (1.0, 1.0), (1e-3, 1e6)):
        assert _create(g, rho_min, ratio_min) == want, (rho_min, ratio_min)
    if g.device_count() <= 0:
        with pytest.raises(g.DvbtError) as e:
            g.Scanner()
        assert "no CPU fallback" in str(e.value)
        with pytest.raises(g.DvbtError):
            g.Scanner.detect(np.zeros(16, np.complex64))


BAD = {
    "negative rho_min": dict(rho_min=-0.1),
    "rho_min above 1": dict(rho_min=1.5),
    "rho_min NaN": dict(rho_min=math.nan),
    "rho_min inf": dict(rho_min=math.inf),
    "ratio_min below 1": dict(ratio_min=0.5),
    "negative ratio_min": dict(ratio_min=-2.0),
    "ratio_min NaN": dict(ratio_min=math.nan),
    "ratio_min inf": dict(ratio_min=math.inf),
    "negative device": dict(device=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, **BAD[name]) == (-1, False), name
    assert g.lib().dvbt_last_error()
    with pytest.raises(g.DvbtError):
        g.Scanner(**BAD[name])
    if "device" not in BAD[name]:
        with pytest.raises(g.DvbtError):
            g.scan_evaluate([0] * 8, [None] * 8, [None] * 8, 0, **BAD[name])


def test_a_device_beyond_the_last_is_refused(g):
    # -1 where there are some, -2 where there is none at all
    assert _create(g, device=1 << 20) == ((-1 if g.device_count() > 0 else -2), False)


def test_null_arguments_are_refused(g):
    from gr_dvbt_amd.binding import _scan_lib
    L = _scan_lib()
    h = C.c_void_p()
    assert L.dvbt_scan_create(None, C.byref(h)) == -1
    assert L.dvbt_scan_create(C.byref(g.ScanParams(0, 0.0, 0.0)), None) == -1
    assert L.dvbt_scan_push(None, None, 0) == -1
    assert L.dvbt_scan_push_device(None, None, 0, None) == -1
    assert L.dvbt_scan_read(None, C.byref(g.ScanResult())) == -1
    assert L.dvbt_scan_accumulators(None, 0, None, None, 0) == -1
    assert L.dvbt_scan_reset(None) == -1
    L.dvbt_scan_destroy(None)
    r, p, J = g.ScanResult(), g.ScanParams(0, 0.0, 0.0), (C.c_int64 * 8)()
    PD = C.POINTER(C.c_double)
    assert L.dvbt_scan_evaluate(None, J, (PD * 8)(), (PD * 8)(), 0, 0, C.byref(r)) == -1
    assert L.dvbt_scan_evaluate(C.byref(p), None, (PD * 8)(), (PD * 8)(), 0, 0, C.byref(r)) == -1
    assert L.dvbt_scan_evaluate(C.byref(p), J, None, (PD * 8)(), 0, 0, C.byref(r)) == -1
    assert L.dvbt_scan_evaluate(C.byref(p), J, (PD * 8)(), (PD * 8)(), 0, 0, None) == -1
    assert L.dvbt_scan_evaluate(C.byref(p), J, (PD * 8)(), (PD * 8)(), 0, 0, C.byref(r)) == 0      # no symbols: no accumulators needed
    assert (r.detected, r.mode, r.guard) == (0, -1, -1) and list(r.rho) == [0.0] * 8
    J[3] = 1
    assert L.dvbt_scan_evaluate(C.byref(p), J, (PD * 8)(), (PD * 8)(), 0, 0, C.byref(r)) == -1     # symbols without accumulators
    J[3] = -1
    assert L.dvbt_scan_evaluate(C.byref(p), J, (PD * 8)(), (PD * 8)(), 0, 0, C.byref(r)) == -1
    with pytest.raises(g.DvbtError):
        g.scan_evaluate([1] * 8, [np.zeros(5, np.complex128)] * 8, [np.zeros(5)] * 8, 0)             # not S bins


# ---------------------------------------------------------------------------------------------- dvbt_scan_evaluate against the model's evaluation

def _signal(h, n, seed, snr_db=6.0, cfo=0.21, start=123):
    """a synthetic OFDM-like stream for hypothesis h: Gaussian useful parts with their last G samples repeated in front, a carrier offset and noise"""
    N, G, S = scanref.dims(h)
    rng = np.random.RandomState(seed)
    nsym = (n + start) // S + 2
    u = (rng.randn(nsym, N) + 1j * rng.randn(nsym, N)) / np.sqrt(2.0)
    x = np.concatenate([u[:, N - G:], u], axis=1).reshape(-1)[S - start:][:n]
    x = x * np.exp(2j * np.pi * cfo / N * np.arange(n))
    x = x + 10.0 ** (-snr_db / 20.0) * (rng.randn(n) + 1j * rng.randn(n)) / np.sqrt(2.0)
    return x.astype(np.complex64)


def _folded(x):
    f = [scanref.fold32(x, h) for h in range(8)]
    return [v[0] for v in f], [v[1] for v in f], [v[2] for v in f]


def _same(got, want):
    assert (int(got.detected), got.mode, got.guard) == (want["detected"], want["mode"], want["guard"])
    assert got.symbol_start == want["symbol_start"] and got.symbols == want["symbols"]
    assert (got.samples_pushed, got.nonfinite) == (want["samples_pushed"], want["nonfinite"])
    for h in range(8):
        for a, b in ((got.rho[h], want["rho"][h]), (got.cfo[h], want["cfo"][h])):
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b), (h, a, b)


@pytest.fixture(scope="module")
def folded():
    """{h: (J, A, E)} of a synthetic signal of hypotheses 2 and 4, SCAN_MIN_SAMPLES + 1000 samples"""
    return {h: _folded(_signal(h, scanref.MIN_SAMPLES + 1000, 7 + h)) for h in (2, 4)}


@pytest.mark.parametrize("h", (2, 4))
def test_evaluate_is_the_models_evaluation(g, folded, h):
    J, A, E = folded[h]
    n = scanref.MIN_SAMPLES + 1000
    want = scanref.evaluate(J, A, E, n)
    assert (want["detected"], want["mode"], want["guard"]) == (1, h >> 2, h & 3), want["rho"]
    assert abs(want["cfo"][h] - 0.21) < 0.01 and want["symbol_start"][h] == 123
    _same(g.scan_evaluate(J, A, E, n), want)
    # thresholds the signal does not meet, and non-finite samples: the same figures, no verdict
    for kw in (dict(rho_min=0.999), dict(ratio_min=1e5), dict(nonfinite=3)):
        want = scanref.evaluate(J, A, E, n, **kw)
        assert want["detected"] == 0
        _same(g.scan_evaluate(J, A, E, n, **kw), want)


def test_too_few_symbols_give_no_verdict(g, folded):
    J, A, E = folded[2]
    J = list(J)
    J[7] = 7
    want = scanref.evaluate(J, A, E, scanref.MIN_SAMPLES - 1)
    assert want["detected"] == 0 and want["best"] == 2
    _same(g.scan_evaluate(J, A, E, scanref.MIN_SAMPLES - 1), want)
    J[7] = 0                                                  # a hypothesis without symbols needs no accumulators and reads 0
    A, E = list(A), list(E)
    A[7] = E[7] = None
    got = g.scan_evaluate(J, A, E, 100)
    assert not got.detected and got.rho[7] == 0.0 and got.rho[2] > 0.5


def _exact(h, scale=1.0):
    """accumulators whose evaluation is exact: A = 1 on the first G bins and -G / N on the rest (the mean is exactly 0, C[0] = G is the peak), E = 1
    (Phi = G): rho = 2 scale at every hypothesis"""
    N, G, S = scanref.dims(h)
    a = np.full(S, -G / N, np.complex128)
    a[:G] = 1.0
    return a * scale, np.ones(S)


def test_equal_rho_picks_the_smallest_hypothesis(g):
    J = [8] * 8
    A, E = [_exact(h)[0] for h in range(8)], [_exact(h)[1] for h in range(8)]
    want = scanref.evaluate(J, A, E, scanref.MIN_SAMPLES, ratio_min=1.0)
    assert want["rho"] == [2.0] * 8 and (want["best"], want["runner_up"]) == (0, 1) and want["symbol_start"] == [0] * 8
    assert (want["detected"], want["mode"], want["guard"]) == (1, 0, 0)
    _same(g.scan_evaluate(J, A, E, scanref.MIN_SAMPLES, ratio_min=1.0), want)
    assert scanref.evaluate(J, A, E, scanref.MIN_SAMPLES)["detected"] == 0 and not g.scan_evaluate(J, A, E, scanref.MIN_SAMPLES).detected   # no lead
    for h in (0, 1, 2, 5):
        A[h] = _exact(h, 0.5)[0]
    want = scanref.evaluate(J, A, E, scanref.MIN_SAMPLES, ratio_min=1.0)
    assert (want["best"], want["runner_up"], want["mode"], want["guard"]) == (3, 4, 0, 3)
    _same(g.scan_evaluate(J, A, E, scanref.MIN_SAMPLES, ratio_min=1.0), want)


def test_a_nan_accumulator_gives_no_verdict(g, folded):
    J, A, E = folded[4]
    n = scanref.MIN_SAMPLES + 1000
    for which, where in (("A", 3), ("A", 4), ("E", 0), ("E", 4)):
        A2, E2 = [a.copy() for a in A], [e.copy() for e in E]
        (A2 if which == "A" else E2)[where][scanref.dims(where)[2] - 1] = math.nan
        want = scanref.evaluate(J, A2, E2, n)
        assert want["detected"] == 0 and math.isnan(want["rho"][where])
        got = g.scan_evaluate(J, A2, E2, n)
        assert not got.detected and (got.mode, got.guard) == (-1, -1)
        _same(got, want)
