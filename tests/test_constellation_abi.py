"""CPU-side checks of the constellation analyser's C ABI (include/dvbt_hip.h, dvbt_constellation_*): exported, laid out as the binding says, every parameter
checked before the device is asked for, no CPU fallback.  (What a live handle refuses -- null or misaligned rows, too many rows, a cap too small -- is in
tests/test_gpu_constellation_block.py: there is no handle without a device.)"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvbt_constellation_create", "dvbt_constellation_push", "dvbt_constellation_push_device", "dvbt_constellation_read", "dvbt_constellation_reset",
           "dvbt_constellation_destroy")
P_FIELDS = ("device", "constellation", "hierarchy", "row_length")
R_FIELDS = ("rows_pushed", "cells", "nonfinite", "clipped", "points", "levels", "alpha", "span")
PT_FIELDS = ("n", "sum_re", "sum_im", "sum_re_im", "sum_re2", "sum_im2")
CA_FIELDS = ("n", "signal", "error")


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _create(g, constellation=2, hierarchy=0, row_length=1512, device=0):
    L = g.lib()
    L.dvbt_constellation_create.argtypes = [C.POINTER(g.ConstellationParams), C.POINTER(C.c_void_p)]
    L.dvbt_constellation_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_constellation_create(C.byref(g.ConstellationParams(device, constellation, hierarchy, row_length)), C.byref(h))
    if h.value:
        L.dvbt_constellation_destroy(h)
    return r, bool(h.value)


def test_every_constellation_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    for name in ("Constellation", "ConstellationReading", "ConstellationParams", "ConstellationResult", "constellation_grid", "POINT_DTYPE", "CARRIER_DTYPE"):
        assert hasattr(g, name)
    assert g.CONSTELLATION_GRID == 128


def test_constellation_structs_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    structs = (("dvbt_constellation_params", P_FIELDS), ("dvbt_constellation_result", R_FIELDS), ("dvbt_constellation_point", PT_FIELDS),
               ("dvbt_constellation_carrier", CA_FIELDS))
    args = ", ".join(", ".join([f"sizeof({s})"] + [f"offsetof({s}, {f})" for f in fields]) for s, fields in structs)
    n = sum(1 + len(f) for _, f in structs) + 1
    fmt = " ".join(["%zu"] * n)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}, (size_t)DVBT_CONSTELLATION_GRID); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, R = g.ConstellationParams, g.ConstellationResult
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in P_FIELDS] + [C.sizeof(R)] + [getattr(R, f).offset for f in R_FIELDS]
    want += [g.POINT_DTYPE.itemsize] + [g.POINT_DTYPE.fields[f][1] for f in PT_FIELDS]
    want += [g.CARRIER_DTYPE.itemsize] + [g.CARRIER_DTYPE.fields[f][1] for f in CA_FIELDS] + [g.CONSTELLATION_GRID]
    assert got == want
    assert want == [16, 0, 4, 8, 12, 48, 0, 8, 16, 24, 32, 36, 40, 44, 48, 0, 8, 16, 24, 32, 40, 24, 0, 8, 16, 128]


GOOD = [(0, 0, 1512), (1, 0, 1), (2, 0, 6048), (1, 1, 8192), (2, 1, 63), (1, 2, 257), (2, 2, 1512), (1, 3, 6048), (2, 3, 64)]


def test_constellation_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    for c, h, p in GOOD:
        assert _create(g, c, h, p) == (-2, False), (c, h, p)
    with pytest.raises(g.DvbtError) as e:
        g.Constellation(g.QAM64)
    assert "no CPU fallback" in str(e.value)


BAD = {
    "constellation 3": dict(constellation=3),
    "negative constellation": dict(constellation=-1),
    "hierarchy 4": dict(hierarchy=4),
    "negative hierarchy": dict(hierarchy=-1),
    "QPSK with alpha 1": dict(constellation=0, hierarchy=1),
    "QPSK with alpha 2": dict(constellation=0, hierarchy=2),
    "QPSK with alpha 4": dict(constellation=0, hierarchy=3),
    "row_length 0": dict(row_length=0),
    "row_length 8193": dict(row_length=8193),
    "negative row_length": dict(row_length=-5),
    "negative device": dict(device=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, **BAD[name]) == (-1, False), name
    assert g.lib().dvbt_last_error()
    with pytest.raises(g.DvbtError):
        g.Constellation(**{"constellation": g.QAM64, **BAD[name]})


def test_a_device_beyond_the_last_is_refused(g):
    # -1 where there are some, -2 where there is none at all
    assert _create(g, device=1 << 20) == ((-1 if g.device_count() > 0 else -2), False)


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_constellation_create.argtypes = [C.POINTER(g.ConstellationParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_constellation_create(None, C.byref(h)) == -1
    assert L.dvbt_constellation_create(C.byref(g.ConstellationParams(0, 2, 0, 1512)), None) == -1
    L.dvbt_constellation_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    assert L.dvbt_constellation_push(None, None, 0) == -1
    L.dvbt_constellation_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.dvbt_constellation_push_device(None, None, 0, None) == -1
    L.dvbt_constellation_read.argtypes = [C.c_void_p, C.POINTER(g.ConstellationResult), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    assert L.dvbt_constellation_read(None, C.byref(g.ConstellationResult()), None, None, 0, None, 0) == -1
    L.dvbt_constellation_reset.argtypes = [C.c_void_p]
    assert L.dvbt_constellation_reset(None) == -1
    L.dvbt_constellation_destroy.argtypes = [C.c_void_p]
    L.dvbt_constellation_destroy(None)
