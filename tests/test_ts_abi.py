"""CPU-side checks of the transport-stream analyser's C ABI (include/dvbt_hip.h, dvbt_ts_*): exported, laid out as the binding says, every parameter checked
before the device is asked for, no CPU fallback.  (What a live handle refuses -- a null buffer, a cap too small -- is in tests/test_gpu_ts_block.py: there
is no handle without a device.)"""
import ctypes as C
import os
import subprocess

import pytest

import tsref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvbt_ts_create", "dvbt_ts_push", "dvbt_ts_push_device", "dvbt_ts_read", "dvbt_ts_reset", "dvbt_ts_destroy")
P_FIELDS = ("device", "max_packets")


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _create(g, max_packets=4096, device=0):
    L = g.lib()
    L.dvbt_ts_create.argtypes = [C.POINTER(g.TsParams), C.POINTER(C.c_void_p)]
    L.dvbt_ts_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_ts_create(C.byref(g.TsParams(device, max_packets)), C.byref(h))
    if h.value:
        L.dvbt_ts_destroy(h)
    return r, bool(h.value)


def test_every_ts_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    for name in ("TsAnalyser", "TsReading", "TsParams", "TsResult", "TS_PID_DTYPE", "ts_align", "TS_TILE"):
        assert hasattr(g, name)
    assert (g.TS_PACKET, g.TS_PIDS) == (188, 8192)
    assert g.TS_PID_DTYPE == tsref.PID_DTYPE and tuple(f for f, _ in g.TsResult._fields_) == tsref.TOTALS, "the model speaks of the binding's fields"


def test_ts_structs_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    R_FIELDS, PID_FIELDS = tsref.TOTALS, tsref.FIELDS
    structs = (("dvbt_ts_params", P_FIELDS), ("dvbt_ts_result", R_FIELDS), ("dvbt_ts_pid", PID_FIELDS))
    args = ", ".join(", ".join([f"sizeof({s})"] + [f"offsetof({s}, {f})" for f in fields]) for s, fields in structs)
    n = sum(1 + len(f) for _, f in structs) + 3
    fmt = " ".join(["%zu"] * n)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}, (size_t)DVBT_TS_PACKET, (size_t)DVBT_TS_PIDS, (size_t)DVBT_TS_TILE); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, R = g.TsParams, g.TsResult
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in P_FIELDS] + [C.sizeof(R)] + [getattr(R, f).offset for f in R_FIELDS]
    want += [g.TS_PID_DTYPE.itemsize] + [g.TS_PID_DTYPE.fields[f][1] for f in PID_FIELDS] + [g.TS_PACKET, g.TS_PIDS, g.TS_TILE]
    assert got == want
    assert want == [8, 0, 4, 48] + list(range(0, 48, 8)) + [184] + list(range(0, 184, 8)) + [188, 8192, g.TS_TILE]
    assert all(g.TS_PID_DTYPE.fields[f][0] == "int64" for f in PID_FIELDS), "every accumulated quantity is a 64-bit integer"


GOOD = [1, 2, 1023, 1024, 1025, 4096, 1 << 19, (1 << 19) + 1, 1 << 24]


def test_ts_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    for m in GOOD:
        assert _create(g, m) == (-2, False), m
    with pytest.raises(g.DvbtError) as e:
        g.TsAnalyser()
    assert "no CPU fallback" in str(e.value)


BAD = {
    "max_packets 0": dict(max_packets=0),
    "negative max_packets": dict(max_packets=-1),
    "max_packets above 2^24": dict(max_packets=(1 << 24) + 1),
    "negative device": dict(device=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, **BAD[name]) == (-1, False), name
    assert g.lib().dvbt_last_error()
    with pytest.raises(g.DvbtError):
        g.TsAnalyser(**BAD[name])


def test_a_device_beyond_the_last_is_refused(g):
    # -1 where there are some, -2 where there is none at all
    assert _create(g, device=1 << 20) == ((-1 if g.device_count() > 0 else -2), False)


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_ts_create.argtypes = [C.POINTER(g.TsParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_ts_create(None, C.byref(h)) == -1
    assert L.dvbt_ts_create(C.byref(g.TsParams(0, 4096)), None) == -1
    L.dvbt_ts_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    assert L.dvbt_ts_push(None, None, 0) == -1
    L.dvbt_ts_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.dvbt_ts_push_device(None, None, 0, None) == -1
    L.dvbt_ts_read.argtypes = [C.c_void_p, C.POINTER(g.TsResult), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    assert L.dvbt_ts_read(None, C.byref(g.TsResult()), None, 0, None) == -1
    L.dvbt_ts_reset.argtypes = [C.c_void_p]
    assert L.dvbt_ts_reset(None) == -1
    L.dvbt_ts_destroy.argtypes = [C.c_void_p]
    L.dvbt_ts_destroy(None)
