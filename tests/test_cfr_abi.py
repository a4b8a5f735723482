"""CPU-side checks of the crest-factor reduction block's C ABI (include/dvbt_hip.h, dvbt_cfr_*): exported, laid out as the binding says, every parameter
checked before the device is asked for, no CPU fallback.  (What a live handle refuses -- a length that cuts a symbol, an overlap, a null buffer -- is in
tests/test_gpu_cfr_block.py: there is no handle without a device.)"""
import ctypes as C
import os
import subprocess

import pytest

import cfrref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvbt_cfr_create", "dvbt_cfr_run", "dvbt_cfr_run_device", "dvbt_cfr_read", "dvbt_cfr_reset", "dvbt_cfr_destroy")
P_FIELDS = ("transmission_mode", "guard_interval", "threshold", "iterations", "oversampling", "keep", "first_symbol", "device")
GOOD = dict(transmission_mode=0, guard_interval=0, threshold=0.05, iterations=4, oversampling=2, keep=3, first_symbol=0, device=0)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _create(g, **kw):
    L = g.lib()
    L.dvbt_cfr_create.argtypes = [C.POINTER(g.CfrParams), C.POINTER(C.c_void_p)]
    L.dvbt_cfr_destroy.argtypes = [C.c_void_p]
    p = g.CfrParams(**dict(GOOD, **kw))
    h = C.c_void_p()
    r = L.dvbt_cfr_create(C.byref(p), C.byref(h))
    if h.value:
        L.dvbt_cfr_destroy(h)
    return r, bool(h.value)


def test_every_cfr_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    for name in ("Cfr", "CfrParams", "CfrResult", "CfrReading", "KEEP_PILOTS", "KEEP_TPS"):
        assert hasattr(g, name)
    assert (g.KEEP_PILOTS, g.KEEP_TPS) == (cfrref.KEEP_PILOTS, cfrref.KEEP_TPS) == (1, 2)
    assert g.CFR_FIELDS == cfrref.FIELDS == tuple(f for f, _ in g.CfrResult._fields_), "the model speaks of the binding's fields"
    assert g.Cfr.threshold_for(7.0, 2.5e-6) == cfrref.threshold_for(7.0, 2.5e-6) == pytest.approx((2.5e-6 * 10 ** 0.7) ** 0.5)


def test_cfr_structs_have_the_headers_layout(g, tmp_path):
    R_FIELDS = cfrref.FIELDS
    structs = (("dvbt_cfr_params", P_FIELDS), ("dvbt_cfr_result", R_FIELDS))
    args = ", ".join(", ".join([f"sizeof({s})"] + [f"offsetof({s}, {f})" for f in fields]) for s, fields in structs)
    n = sum(1 + len(f) for _, f in structs) + 2
    fmt = " ".join(["%zu"] * n)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}, (size_t)DVBT_CFR_KEEP_PILOTS, (size_t)DVBT_CFR_KEEP_TPS); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, R = g.CfrParams, g.CfrResult
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in P_FIELDS] + [C.sizeof(R)] + [getattr(R, f).offset for f in R_FIELDS] + [g.KEEP_PILOTS, g.KEEP_TPS]
    assert got == want
    assert want == [40, 0, 4, 8, 12, 16, 20, 24, 32, 40, 0, 8, 16, 24, 32, 1, 2]


def test_cfr_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    for kw in (dict(), dict(transmission_mode=1, guard_interval=3), dict(iterations=0), dict(iterations=8, oversampling=4), dict(oversampling=1, keep=0),
               dict(first_symbol=1 << 40), dict(threshold=1e-30), dict(threshold=3e38)):
        assert _create(g, **kw) == (-2, False), kw
    with pytest.raises(g.DvbtError) as e:
        g.Cfr(g.T2k, g.G1_32, 0.05)
    assert "no CPU fallback" in str(e.value)


BAD = {
    "mode below": dict(transmission_mode=-1),
    "mode above": dict(transmission_mode=2),
    "guard below": dict(guard_interval=-1),
    "guard above": dict(guard_interval=4),
    "threshold 0": dict(threshold=0.0),
    "threshold negative": dict(threshold=-0.05),
    "threshold nan": dict(threshold=float("nan")),
    "threshold inf": dict(threshold=float("inf")),
    "iterations negative": dict(iterations=-1),
    "iterations 9": dict(iterations=9),
    "oversampling 0": dict(oversampling=0),
    "oversampling 3": dict(oversampling=3),
    "oversampling 8": dict(oversampling=8),
    "oversampling negative": dict(oversampling=-2),
    "keep bit 2": dict(keep=4),
    "keep negative": dict(keep=-1),
    "first_symbol negative": dict(first_symbol=-1),
    "negative device": dict(device=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, **BAD[name]) == (-1, False), name
    assert g.lib().dvbt_last_error()
    kw = dict(GOOD, **BAD[name])
    with pytest.raises(g.DvbtError):
        g.Cfr(kw.pop("transmission_mode"), kw.pop("guard_interval"), kw.pop("threshold"), **kw)


def test_a_device_beyond_the_last_is_refused(g):
    # -1 where there are some, -2 where there is none at all
    assert _create(g, device=1 << 20) == ((-1 if g.device_count() > 0 else -2), False)


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_cfr_create.argtypes = [C.POINTER(g.CfrParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_cfr_create(None, C.byref(h)) == -1
    assert L.dvbt_cfr_create(C.byref(g.CfrParams(**GOOD)), None) == -1
    L.dvbt_cfr_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.dvbt_cfr_run(None, None, 0, None) == -1
    L.dvbt_cfr_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert L.dvbt_cfr_run_device(None, None, 0, None, None) == -1
    L.dvbt_cfr_read.argtypes = [C.c_void_p, C.POINTER(g.CfrResult)]
    assert L.dvbt_cfr_read(None, C.byref(g.CfrResult())) == -1
    L.dvbt_cfr_reset.argtypes = [C.c_void_p]
    assert L.dvbt_cfr_reset(None) == -1
    L.dvbt_cfr_destroy.argtypes = [C.c_void_p]
    L.dvbt_cfr_destroy(None)
