"""CPU-side checks of the tuner block's C ABI (include/dvbt_hip.h, dvbt_tuner_*): exported, laid out as the binding says, every parameter checked before
the device is asked for, no CPU fallback, and the host's output count and designed prototype equal to the model's (tests/tunerref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tunerref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNER_SYMBOLS = ("dvbt_tuner_design", "dvbt_tuner_outputs", "dvbt_tuner_create", "dvbt_tuner_get_taps", "dvbt_tuner_info", "dvbt_tuner_outputs_for",
                 "dvbt_tuner_run", "dvbt_tuner_run_device", "dvbt_tuner_reset", "dvbt_tuner_destroy")
FIELDS = ("format", "interpolation", "decimation", "swap_iq", "shift", "scale", "pass_edge", "stop_edge", "atten_db", "first_in", "device")
DESC_FIELDS = ("interpolation", "decimation", "ntaps", "nt", "delay_num", "delay_den", "phase_inc")
FAR = 2 ** 40 + 3
RATIOS = [(1, 1), (32, 35), (8, 7), (16, 35), (1, 8), (128, 175)]


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _params(g, format=1, interpolation=32, decimation=35, **kw):
    return g.TunerParams.of(format, interpolation, decimation, **kw)


def _raw_params(g, **kw):
    """a good struct with single fields overwritten behind the Python layer's defaults"""
    p = _params(g)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _create(g, p, taps=None):
    L = g.lib()
    L.dvbt_tuner_create.argtypes = [C.POINTER(g.TunerParams), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.dvbt_tuner_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    if taps is None:
        r = L.dvbt_tuner_create(C.byref(p), None, 0, C.byref(h))
    else:
        t = np.ascontiguousarray(taps, np.float32)
        r = L.dvbt_tuner_create(C.byref(p), t.ctypes.data_as(C.c_void_p), len(t), C.byref(h))
    if h.value:
        L.dvbt_tuner_destroy(h)
    return r, bool(h.value)


def _outputs(g, p, n, ntaps=0):
    L = g.lib()
    L.dvbt_tuner_outputs.argtypes = [C.POINTER(g.TunerParams), C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    v = C.c_int64(-7)
    return L.dvbt_tuner_outputs(C.byref(p), ntaps, n, C.byref(v)), v.value


def _design(g, p):
    L = g.lib()
    L.dvbt_tuner_design.argtypes = [C.POINTER(g.TunerParams), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    n = C.c_int(-7)
    return L.dvbt_tuner_design(C.byref(p), None, 0, C.byref(n)), n.value


def test_every_tuner_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in TUNER_SYMBOLS if not hasattr(L, n)]
    assert not missing, missing


def test_tuner_structs_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    n = len(FIELDS) + len(DESC_FIELDS) + 6
    fmt = " ".join(["%zu"] * n)
    offs = ", ".join([f"offsetof(dvbt_tuner_params, {f})" for f in FIELDS] + [f"offsetof(dvbt_tuner_desc, {f})" for f in DESC_FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dvbt_tuner_params), sizeof(dvbt_tuner_desc), (size_t)DVBT_IQ_CF32, (size_t)DVBT_IQ_CS16, '
                   f'(size_t)DVBT_IQ_CS8, (size_t)DVBT_IQ_CU8, {offs}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, D = g.TunerParams, g.TunerDesc
    want = ([C.sizeof(P), C.sizeof(D), g.IQ_CF32, g.IQ_CS16, g.IQ_CS8, g.IQ_CU8] + [getattr(P, f).offset for f in FIELDS]
            + [getattr(D, f).offset for f in DESC_FIELDS])
    assert got == want
    assert want[:2] == [72, 40] and want[6:6 + len(FIELDS)] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert (g.IQ_BYTES, [d.itemsize for d in g.IQ_DTYPES]) == ((8, 4, 2, 2), [8, 2, 1, 1])


def test_tuner_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _create(g, _params(g)) == (-2, False)
    for fmt in range(4):
        assert _create(g, _params(g, fmt, 64, 70, shift=-0.5, swap_iq=True, first_in=2 ** 48)) == (-2, False)
    assert _create(g, _params(g, 0, 1, 1), taps=[1.0]) == (-2, False)
    assert _create(g, _params(g, 2, 128, 175, atten_db=90, shift=0.5)) == (-2, False)
    assert _create(g, _params(g, 3, 1, 8, atten_db=40, pass_edge=0.3, stop_edge=1.0)) == (-2, False)
    with pytest.raises(g.DvbtError) as e:
        g.Tuner(g.IQ_CS16, 32, 35)
    assert "no CPU fallback" in str(e.value)
    with pytest.raises(g.DvbtError) as e:
        g.Tuner.for_capture(10e6, g.IQ_CS8, offset_hz=250e3)
    assert "no CPU fallback" in str(e.value)


def test_for_capture_ratios(g):
    from fractions import Fraction
    for rate, want in ((8e6, (8, 7)), (10e6, (32, 35)), (12.5e6, (128, 175)), (16e6, (4, 7)), (20e6, (16, 35)), (25e6, (64, 175))):
        r = Fraction(64_000_000 * 8, 56) / Fraction(rate)
        assert (r.numerator, r.denominator) == want
    with pytest.raises(ValueError):
        g.Tuner.for_capture(100e6, g.IQ_CS16)                  # M / L = 175 / 16 > 8
    with pytest.raises(ValueError):
        g.Tuner.for_capture(10e6 + 1, g.IQ_CS16)               # no small ratio
    with pytest.raises(ValueError):
        g.TunerParams.of(4, 1, 1)


BAD = {
    "format 4": dict(format=4),
    "negative format": dict(format=-1),
    "interpolation 0": dict(interpolation=0),
    "negative decimation": dict(decimation=-35),
    "interpolation 129": dict(interpolation=129, decimation=128),
    "decimation 1025": dict(interpolation=128, decimation=1025),
    "decimation above 8 interpolations": dict(interpolation=7, decimation=57),
    "swap_iq 2": dict(swap_iq=2),
    "nan shift": dict(shift=float("nan")),
    "infinite shift": dict(shift=float("inf")),
    "shift above one half": dict(shift=0.5000001),
    "zero scale": dict(scale=0.0),
    "nan scale": dict(scale=float("nan")),
    "infinite scale": dict(scale=float("inf")),
    "atten 39": dict(atten_db=39.0),
    "atten 91": dict(atten_db=91.0),
    "nan atten": dict(atten_db=float("nan")),
    "zero pass": dict(pass_edge=0.0),
    "pass at stop": dict(pass_edge=0.5, stop_edge=0.5),
    "stop above 1": dict(stop_edge=1.01),
    "nan stop": dict(stop_edge=float("nan")),
    "negative first_in": dict(first_in=-1),
    "first_in beyond 2^48": dict(first_in=2 ** 48 + 1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    p = _raw_params(g, **BAD[name])
    assert _create(g, p) == (-1, False), name
    assert g.lib().dvbt_last_error()
    assert _create(g, p, taps=np.ones(33)) == (-1, False)
    assert _outputs(g, p, 1000) == (-1, -7)
    assert _outputs(g, p, 1000, ntaps=33) == (-1, -7)
    assert _design(g, p) == (-1, -7)
    with pytest.raises(g.DvbtError):
        g.tuner_outputs(p, 1000)
    with pytest.raises(g.DvbtError):
        g.tuner_design(p)


def test_bad_prototypes_are_refused_before_the_device_is_asked_for(g):
    good = _params(g)
    assert _create(g, _params(g, 1, 1, 2), taps=np.ones(321)) == (-1, False)    # nt = 321
    assert _outputs(g, _params(g, 1, 1, 2), 10, ntaps=321) == (-1, -7) and _outputs(g, _params(g, 1, 1, 2), 10, ntaps=320) == (0, 5)
    assert _create(g, _params(g, 1, 128, 175), taps=np.ones(128 * 64 + 1)) == (-1, False)   # L nt = 128 * 65
    assert _create(g, good, taps=[1.0, float("nan")]) == (-1, False)
    assert _create(g, good, taps=[1.0, float("inf")]) == (-1, False)
    assert _create(g, good, taps=np.zeros(0)) == (-1, False)
    assert _outputs(g, good, 10, ntaps=-1) == (-1, -7)
    assert _outputs(g, good, 10, ntaps=32 * 256 + 1) == (-1, -7)                # L nt = 32 * 257
    assert _outputs(g, good, 10, ntaps=32 * 256)[0] == 0
    # a design that cannot fit: 90 dB over a transition of 0.01 / 8 of the prototype's rate at 1/8 needs more than 320 taps per branch
    tight = _params(g, 1, 1, 8, pass_edge=0.45, stop_edge=0.46, atten_db=90)
    assert _create(g, tight) == (-1, False) and _design(g, tight) == (-1, -7) and _outputs(g, tight, 10) == (-1, -7)
    # no room in front of the capture's first image: 8/7 with pass 0.45 leaves stop = 0.875 - 0.45 < pass
    assert _create(g, _params(g, 1, 8, 7, pass_edge=0.45)) == (-1, False)
    # the caller's taps do not need the design to fit
    assert _create(g, tight, taps=np.ones(9))[0] in (0, -2)


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_tuner_create.argtypes = [C.POINTER(g.TunerParams), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_tuner_create(None, None, 0, C.byref(h)) == -1
    assert L.dvbt_tuner_create(C.byref(_params(g)), None, 0, None) == -1
    L.dvbt_tuner_outputs.argtypes = [C.POINTER(g.TunerParams), C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    v = C.c_int64()
    assert L.dvbt_tuner_outputs(None, 0, 0, C.byref(v)) == -1
    assert L.dvbt_tuner_outputs(C.byref(_params(g)), 0, 0, None) == -1
    assert L.dvbt_tuner_outputs(C.byref(_params(g)), 0, -1, C.byref(v)) == -1
    assert L.dvbt_tuner_outputs(C.byref(_params(g)), 0, 2 ** 48 + 1, C.byref(v)) == -1
    L.dvbt_tuner_design.argtypes = [C.POINTER(g.TunerParams), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    n = C.c_int()
    assert L.dvbt_tuner_design(None, None, 0, C.byref(n)) == -1
    assert L.dvbt_tuner_design(C.byref(_params(g)), None, 0, None) == -1
    buf = np.zeros(4, np.float32)
    assert L.dvbt_tuner_design(C.byref(_params(g)), buf.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == -4      # DVBT_ERR_CAPACITY
    assert not buf.any()
    z = C.c_size_t()
    L.dvbt_tuner_outputs_for.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    assert L.dvbt_tuner_outputs_for(None, 0, C.byref(z)) == -1
    L.dvbt_tuner_get_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    assert L.dvbt_tuner_get_taps(None, None, 0, C.byref(n)) == -1
    L.dvbt_tuner_info.argtypes = [C.c_void_p, C.c_void_p]
    assert L.dvbt_tuner_info(None, None) == -1
    L.dvbt_tuner_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    assert L.dvbt_tuner_run(None, None, 0, None, 0, C.byref(z)) == -1
    L.dvbt_tuner_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    assert L.dvbt_tuner_run_device(None, None, 0, None, 0, C.byref(z), None) == -1
    L.dvbt_tuner_reset.argtypes = [C.c_void_p]
    assert L.dvbt_tuner_reset(None) == -1


# about 2,000 totals: the first 201, those around 2^31 and a spread between
TOTALS = list(range(0, 201)) + [2 ** 31 + d for d in range(-20, 21)] + [1000 * i * i + 7 * i for i in range(15, 15 + 1760)]


@pytest.mark.parametrize("ratio", RATIOS, ids=[f"{a}/{b}" for a, b in RATIOS])
def test_output_counts_equal_the_models(g, ratio):
    L, M = ratio
    assert 1900 <= len(TOTALS) <= 2100 and max(TOTALS) > 2 ** 31
    for k in (1, 2):                                                             # the unreduced ratio counts the same
        for first_in in (0, FAR):
            p = _params(g, 1, k * L, k * M, first_in=first_in)
            want = [tunerref.outputs(n, L, M, first_in) for n in TOTALS]
            assert [g.tuner_outputs(p, n, ntaps=33) for n in TOTALS] == want, (k, first_in)
    p = _params(g, 1, L, M, first_in=7)
    assert g.tuner_outputs(p, 100000) == tunerref.outputs(100000, L, M, 7)       # ntaps = 0: the designed prototype decides acceptance only
    # the count is the number of m with first_in <= n(m) < first_in + N
    for first_in in (0, 5):
        for N in (0, 1, 2, 9, 10, 33):
            ms = [m for m in range(0, 8 * (first_in + N) + 8) if first_in <= (m * M) // L < first_in + N]
            assert tunerref.outputs(N, L, M, first_in) == len(ms)


@pytest.mark.parametrize("atten", [40.0, 50.0, 70.0, 90.0])
@pytest.mark.parametrize("ratio", RATIOS[1:] + [(4, 7), (64, 175), (25, 28)], ids=lambda r: f"{r[0]}/{r[1]}")
def test_the_designed_prototype_equals_the_models(g, ratio, atten):
    L, M = ratio
    got = g.tuner_design(_params(g, 1, 2 * L, 2 * M, atten_db=atten))
    want = tunerref.design(L, M, atten_db=atten)
    assert got.dtype == np.float32 and len(got) == len(want) and len(got) % 2 == 1
    # the libm and the numpy of one machine may differ in the last bit of a sine or a square root
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(want).max()
    assert abs(float(got.astype(np.float64).sum()) - L) < 1e-4 * L
    assert (got == got[::-1]).all()


def test_other_edges_reach_the_design(g):
    got = g.tuner_design(_params(g, 1, 32, 35, pass_edge=0.3, stop_edge=0.7))
    want = tunerref.design(32, 35, 0.3, 0.7)
    assert len(got) == len(want) < len(tunerref.design(32, 35))
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(want).max()
