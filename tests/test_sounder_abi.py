"""CPU-side checks of the channel sounder's C ABI (include/dvbt_hip.h, dvbt_sounder_*): exported, laid out as the binding says, every parameter checked
before the device is asked for, no CPU fallback.  (What a live handle refuses -- null or misaligned rows, too many symbols -- is in
tests/test_gpu_sounder_block.py: there is no handle without a device.)"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvbt_sounder_create", "dvbt_sounder_push", "dvbt_sounder_push_device", "dvbt_sounder_read", "dvbt_sounder_reset", "dvbt_sounder_destroy")
P_FIELDS = ("device", "transmission_mode", "window", "first_index")
R_FIELDS = ("symbols_pushed", "groups_used", "groups_skipped", "M", "Kp")


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _create(g, mode=0, window=1, first_index=0, device=0):
    L = g.lib()
    L.dvbt_sounder_create.argtypes = [C.POINTER(g.SounderParams), C.POINTER(C.c_void_p)]
    L.dvbt_sounder_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_sounder_create(C.byref(g.SounderParams(device, mode, window, first_index)), C.byref(h))
    if h.value:
        L.dvbt_sounder_destroy(h)
    return r, bool(h.value)


def test_every_sounder_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    for name in ("Sounder", "SounderReading", "SounderParams", "SounderResult"):
        assert hasattr(g, name)


def test_sounder_structs_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    n = len(P_FIELDS) + 1 + len(R_FIELDS) + 1
    fmt = " ".join(["%zu"] * n)
    poffs = ", ".join(f"offsetof(dvbt_sounder_params, {f})" for f in P_FIELDS)
    roffs = ", ".join(f"offsetof(dvbt_sounder_result, {f})" for f in R_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dvbt_sounder_params), {poffs}, sizeof(dvbt_sounder_result), {roffs}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, R = g.SounderParams, g.SounderResult
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in P_FIELDS] + [C.sizeof(R)] + [getattr(R, f).offset for f in R_FIELDS]
    assert got == want
    assert want == [16, 0, 4, 8, 12, 32, 0, 8, 16, 24, 28]


def test_sounder_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    for mode in (0, 1):
        for window in (0, 1):
            for first_index in (0, 1, 67):
                assert _create(g, mode, window, first_index) == (-2, False), (mode, window, first_index)
    with pytest.raises(g.DvbtError) as e:
        g.Sounder(g.T2k)
    assert "no CPU fallback" in str(e.value)


BAD = {
    "mode 2": dict(mode=2),
    "negative mode": dict(mode=-1),
    "window 2 (Blackman-Harris is the spectrum analyser's)": dict(window=2),
    "negative window": dict(window=-1),
    "first_index 68": dict(first_index=68),
    "negative first_index": dict(first_index=-1),
    "negative device": dict(device=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, **BAD[name]) == (-1, False), name
    assert g.lib().dvbt_last_error()
    with pytest.raises(g.DvbtError):
        g.Sounder(**{"mode": g.T2k, **BAD[name]})


def test_a_bad_window_name_or_device_is_refused(g):
    with pytest.raises(g.DvbtError):
        g.Sounder(g.T2k, window="blackman-harris")
    # a device beyond the last: -1 where there are some, -2 where there is none at all
    assert _create(g, device=1 << 20) == ((-1 if g.device_count() > 0 else -2), False)


def test_null_arguments_are_refused(g):
    L = g.lib()
    PI = C.POINTER(C.c_int)
    L.dvbt_sounder_create.argtypes = [C.POINTER(g.SounderParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_sounder_create(None, C.byref(h)) == -1
    assert L.dvbt_sounder_create(C.byref(g.SounderParams(0, 0, 1, 0)), None) == -1
    L.dvbt_sounder_push.argtypes = [C.c_void_p, C.c_void_p, PI, PI, PI, C.c_size_t]
    assert L.dvbt_sounder_push(None, None, None, None, None, 0) == -1
    L.dvbt_sounder_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.dvbt_sounder_push_device(None, None, None, None, None, 0, None) == -1
    L.dvbt_sounder_read.argtypes = [C.c_void_p, C.POINTER(g.SounderResult), C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double), C.c_size_t]
    assert L.dvbt_sounder_read(None, C.byref(g.SounderResult()), None, 0, None, 0) == -1
    L.dvbt_sounder_reset.argtypes = [C.c_void_p]
    assert L.dvbt_sounder_reset(None) == -1
    L.dvbt_sounder_destroy.argtypes = [C.c_void_p]
    L.dvbt_sounder_destroy(None)
