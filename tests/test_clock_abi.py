"""CPU-side checks of the sample-clock offset block's C ABI (include/dvbt_hip.h, dvbt_clock_*): exported, laid out as the binding says, every parameter
checked before the device is asked for, no CPU fallback, and the host's output count equal to the model's E (tests/clockref.py)."""
import ctypes as C
import os
import subprocess

import pytest

import clockref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOCK_SYMBOLS = ("dvbt_clock_outputs", "dvbt_clock_create", "dvbt_clock_outputs_for", "dvbt_clock_run", "dvbt_clock_run_device", "dvbt_clock_reset",
                 "dvbt_clock_destroy")
FIELDS = ("ppm", "start", "taps", "first_out", "first_in", "device")
FAR = 2 ** 40 + 3


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _params(g, ppm=37.5, start=8.0, taps=16, first_out=0, first_in=0):
    return g.ClockParams(ppm, start, taps, first_out, first_in, 0)


def _create(g, p):
    L = g.lib()
    L.dvbt_clock_create.argtypes = [C.POINTER(g.ClockParams), C.POINTER(C.c_void_p)]
    L.dvbt_clock_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_clock_create(C.byref(p), C.byref(h))
    if h.value:
        L.dvbt_clock_destroy(h)
    return r, bool(h.value)


def _outputs(g, p, n):
    L = g.lib()
    L.dvbt_clock_outputs.argtypes = [C.POINTER(g.ClockParams), C.c_int64, C.POINTER(C.c_int64)]
    v = C.c_int64(-7)
    return L.dvbt_clock_outputs(C.byref(p), n, C.byref(v)), v.value


def test_every_clock_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in CLOCK_SYMBOLS if not hasattr(L, n)]
    assert not missing, missing


def test_clock_params_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1))
    offs = ", ".join(f"offsetof(dvbt_clock_params, {f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dvbt_clock_params), {offs}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = g.ClockParams
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS]
    assert got == want
    assert want == [48, 0, 8, 16, 24, 32, 40]


def test_clock_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _create(g, _params(g)) == (-2, False)
    assert _create(g, _params(g, ppm=0.0, start=0.0, taps=0)) == (-2, False)
    assert _create(g, _params(g, ppm=-1000.0, start=32.0 + 2.0 ** -40, taps=64, first_out=FAR, first_in=2 ** 48)) == (-2, False)
    with pytest.raises(g.DvbtError) as e:
        g.ClockOffset(10.0)
    assert "no CPU fallback" in str(e.value)


BAD = {
    "nan ppm": dict(ppm=float("nan")),
    "infinite ppm": dict(ppm=float("inf")),
    "ppm above 1000": dict(ppm=1000.5),
    "ppm below -1000": dict(ppm=-1000.5),
    "negative start": dict(start=-0.5),
    "nan start": dict(start=float("nan")),
    "start 2^31": dict(start=2.0 ** 31),
    "taps 24": dict(taps=24),
    "negative taps": dict(taps=-16),
    "negative first_out": dict(first_out=-1),
    "negative first_in": dict(first_in=-1),
    "first_out beyond 2^48": dict(first_out=2 ** 48 + 1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, _params(g, **BAD[name])) == (-1, False), name
    assert g.lib().dvbt_last_error()
    assert _outputs(g, _params(g, **BAD[name]), 1000) == (-1, -7)
    with pytest.raises(g.DvbtError):
        g.clock_outputs(_params(g, **BAD[name]), 1000)


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_clock_create.argtypes = [C.POINTER(g.ClockParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_clock_create(None, C.byref(h)) == -1
    assert L.dvbt_clock_create(C.byref(_params(g)), None) == -1
    L.dvbt_clock_outputs.argtypes = [C.POINTER(g.ClockParams), C.c_int64, C.POINTER(C.c_int64)]
    v = C.c_int64()
    assert L.dvbt_clock_outputs(None, 0, C.byref(v)) == -1
    assert L.dvbt_clock_outputs(C.byref(_params(g)), 0, None) == -1
    assert L.dvbt_clock_outputs(C.byref(_params(g)), -1, C.byref(v)) == -1
    n = C.c_size_t()
    L.dvbt_clock_outputs_for.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    assert L.dvbt_clock_outputs_for(None, 0, C.byref(n)) == -1
    L.dvbt_clock_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    assert L.dvbt_clock_run(None, None, 0, None, 0, C.byref(n)) == -1
    L.dvbt_clock_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    assert L.dvbt_clock_run_device(None, None, 0, None, 0, C.byref(n), None) == -1
    L.dvbt_clock_reset.argtypes = [C.c_void_p]
    assert L.dvbt_clock_reset(None) == -1


# about 2,000 totals: the first 201, those around 2^31 and a spread between
TOTALS = list(range(0, 201)) + [2 ** 31 + d for d in range(-20, 21)] + [1000 * i * i + 7 * i for i in range(15, 15 + 1760)]


@pytest.mark.parametrize("taps", [16, 32, 64])
@pytest.mark.parametrize("ppm", [0.0, 37.5, -37.5, 1000.0, -1000.0])
def test_output_counts_equal_the_models(g, taps, ppm):
    H = taps // 2
    assert 1900 <= len(TOTALS) <= 2100 and max(TOTALS) > 2 ** 31
    for start in (0.0, float(H), H + 0.5, H + 2.0 ** -40):
        for first_out, first_in in ((0, 0), (FAR, clockref.first_in_for(FAR, ppm, start, taps)), (5, FAR), (FAR, 0)):
            p = _params(g, ppm, start, taps, first_out, first_in)
            m0 = clockref.next_output(0, ppm, start, taps, first_out, first_in)
            want = [max(clockref.E(first_in + n, ppm, start, taps), first_out) - m0 for n in TOTALS]
            got = [g.clock_outputs(p, n) for n in TOTALS]
            assert got == want, (start, first_out, first_in)
    # taps = 0 is 16
    assert g.clock_outputs(_params(g, ppm, 8.0, 0), 100000) == clockref.outputs(100000, ppm, 8.0, 16)
