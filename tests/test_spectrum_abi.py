"""CPU-side checks of the spectrum analyser's C ABI (include/dvbt_hip.h, dvbt_spectrum_*): exported, laid out as the binding says, every parameter checked
before the device is asked for, no CPU fallback."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvbt_spectrum_create", "dvbt_spectrum_push", "dvbt_spectrum_push_device", "dvbt_spectrum_read", "dvbt_spectrum_reset", "dvbt_spectrum_destroy")
P_FIELDS = ("device", "fft_size", "hop", "window")
R_FIELDS = ("segments", "samples_pushed", "samples_counted", "nonfinite", "sum_power", "peak_power")


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _create(g, fft_size=2048, hop=0, window=1, device=0):
    L = g.lib()
    L.dvbt_spectrum_create.argtypes = [C.POINTER(g.SpectrumParams), C.POINTER(C.c_void_p)]
    L.dvbt_spectrum_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_spectrum_create(C.byref(g.SpectrumParams(device, fft_size, hop, window)), C.byref(h))
    if h.value:
        L.dvbt_spectrum_destroy(h)
    return r, bool(h.value)


def test_every_spectrum_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    assert g.SPECTRUM_HIST_BINS == 2048
    for name in ("Spectrum", "SpectrumReading", "SpectrumParams", "SpectrumResult"):
        assert hasattr(g, name)


def test_spectrum_structs_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    n = len(P_FIELDS) + 1 + len(R_FIELDS) + 1
    fmt = " ".join(["%zu"] * n) + " %d"
    poffs = ", ".join(f"offsetof(dvbt_spectrum_params, {f})" for f in P_FIELDS)
    roffs = ", ".join(f"offsetof(dvbt_spectrum_result, {f})" for f in R_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dvbt_spectrum_params), {poffs}, sizeof(dvbt_spectrum_result), {roffs}, '
                   'DVBT_SPECTRUM_HIST_BINS); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, R = g.SpectrumParams, g.SpectrumResult
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in P_FIELDS] + [C.sizeof(R)] + [getattr(R, f).offset for f in R_FIELDS]
    assert got[:-1] == want
    assert want == [16, 0, 4, 8, 12, 48, 0, 8, 16, 24, 32, 40]
    assert got[-1] == 2048


def test_spectrum_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    for N in (64, 128, 2048, 8192):
        for hop in (0, N // 8, 3 * N // 8, N):
            for window in (0, 1, 2):
                assert _create(g, N, hop, window) == (-2, False), (N, hop, window)
    with pytest.raises(g.DvbtError) as e:
        g.Spectrum()
    assert "no CPU fallback" in str(e.value)


BAD = {
    "fft_size below 64": dict(fft_size=32),
    "fft_size above 8192": dict(fft_size=16384),
    "fft_size no power of two": dict(fft_size=1000),
    "fft_size 0": dict(fft_size=0),
    "negative fft_size": dict(fft_size=-2048),
    "hop below an eighth": dict(fft_size=2048, hop=255),
    "hop above fft_size": dict(fft_size=2048, hop=2049),
    "negative hop": dict(fft_size=2048, hop=-1024),
    "window 3": dict(window=3),
    "negative window": dict(window=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, **BAD[name]) == (-1, False), name
    assert g.lib().dvbt_last_error()
    with pytest.raises(g.DvbtError):
        g.Spectrum(**BAD[name])


def test_a_bad_window_name_or_device_is_refused(g):
    with pytest.raises(g.DvbtError):
        g.Spectrum(window="kaiser")
    assert _create(g, device=-1) == (-1, False)                # needs no device to be refused
    # a device beyond the last: -1 where there are some, -2 where there is none at all
    assert _create(g, device=1 << 20) == ((-1 if g.device_count() > 0 else -2), False)
    with pytest.raises(g.DvbtError):
        g.Spectrum(device=-1)


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_spectrum_create.argtypes = [C.POINTER(g.SpectrumParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_spectrum_create(None, C.byref(h)) == -1
    assert L.dvbt_spectrum_create(C.byref(g.SpectrumParams(0, 2048, 0, 1)), None) == -1
    L.dvbt_spectrum_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    assert L.dvbt_spectrum_push(None, None, 0) == -1
    L.dvbt_spectrum_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.dvbt_spectrum_push_device(None, None, 0, None) == -1
    L.dvbt_spectrum_read.argtypes = [C.c_void_p, C.POINTER(g.SpectrumResult), C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]
    assert L.dvbt_spectrum_read(None, C.byref(g.SpectrumResult()), None, None) == -1
    L.dvbt_spectrum_reset.argtypes = [C.c_void_p]
    assert L.dvbt_spectrum_reset(None) == -1
    L.dvbt_spectrum_destroy.argtypes = [C.c_void_p]
    L.dvbt_spectrum_destroy(None)
