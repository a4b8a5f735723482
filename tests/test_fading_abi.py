"""CPU-side checks of the fading block's C ABI (include/dvbt_hip.h, dvbt_fading_*): exported, laid out as the binding says, every parameter checked before
the device is asked for, no CPU fallback, and the host's sinusoid table equal to the model's word for word (tests/fadingref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fadingref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADING_SYMBOLS = ("dvbt_fading_table", "dvbt_fading_create", "dvbt_fading_run", "dvbt_fading_run_device", "dvbt_fading_reset", "dvbt_fading_destroy")
FIELDS = ("n_paths", "delay", "los_re", "los_im", "sigma", "doppler", "n_sinusoids", "seed", "first_sample", "device")
FAR = 2 ** 40 + 3
GOOD = ((0, 1.0, 0.0), (7, 0.25 - 0.5j, 0.5), (8192, 0.0, 1.0))


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _params(g, paths=GOOD, doppler=1e-5, n_sinusoids=16, seed=5, first_sample=0):
    return g.FadingParams.of(paths, doppler, n_sinusoids, seed, first_sample, 0)


def _create(g, p):
    L = g.lib()
    L.dvbt_fading_create.argtypes = [C.POINTER(g.FadingParams), C.POINTER(C.c_void_p)]
    L.dvbt_fading_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_fading_create(C.byref(p), C.byref(h))
    if h.value:
        L.dvbt_fading_destroy(h)
    return r, bool(h.value)


def _table(g, p):
    L = g.lib()
    L.dvbt_fading_table.argtypes = [C.POINTER(g.FadingParams), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    inc, ph = (C.c_uint64 * (24 * 32))(), (C.c_uint64 * (24 * 32))()
    for i in range(24 * 32):
        inc[i] = ph[i] = 0xdeadbeef
    r = L.dvbt_fading_table(C.byref(p), inc, ph)
    return r, all(v == 0xdeadbeef for v in inc) and all(v == 0xdeadbeef for v in ph)


def test_every_fading_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in FADING_SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    assert (g.FADING_MAX_PATHS, g.FADING_MAX_DELAY, g.FADING_MAX_SINUSOIDS, g.FADING_KNOT) == (24, 8192, 32, 64)
    assert (fadingref.MAX_PATHS, fadingref.MAX_DELAY, fadingref.MAX_SINUSOIDS, fadingref.KNOT) == (24, 8192, 32, 64)


def test_fading_params_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1)) + " %d %d %d %d"
    offs = ", ".join(f"offsetof(dvbt_fading_params, {f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dvbt_fading_params), {offs}, DVBT_FADING_MAX_PATHS, DVBT_FADING_MAX_DELAY, '
                   'DVBT_FADING_MAX_SINUSOIDS, DVBT_FADING_KNOT); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = g.FadingParams
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS]
    assert got[:-4] == want
    assert want == [432, 0, 4, 100, 196, 292, 392, 400, 408, 416, 424]
    assert got[-4:] == [24, 8192, 32, 64]


def test_fading_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _create(g, _params(g)) == (-2, False)
    assert _create(g, _params(g, paths=((0, 1.0, 0.0),), doppler=0.0, n_sinusoids=0)) == (-2, False)
    assert _create(g, _params(g, paths=tuple((8192, 1j, 2.0) for _ in range(24)), doppler=2.0 ** -12, n_sinusoids=32, seed=2 ** 64 - 1,
                              first_sample=FAR)) == (-2, False)
    with pytest.raises(g.DvbtError) as e:
        g.Fading()
    assert "no CPU fallback" in str(e.value)
    with pytest.raises(g.DvbtError):
        g.Fading.tu6(100.0, rice_k_db=10.0, seed=3)


BAD = {
    "no paths": dict(paths=()),
    "negative delay": dict(paths=((0, 1.0, 0.0), (-1, 0.5, 0.0))),
    "delay 8193": dict(paths=((8193, 1.0, 0.0),)),
    "nan fixed part": dict(paths=((0, float("nan"), 0.0),)),
    "infinite fixed part": dict(paths=((0, complex(0.0, float("inf")), 0.0),)),
    "negative sigma": dict(paths=((0, 1.0, 0.0), (3, 0.0, -0.5))),
    "nan sigma": dict(paths=((0, 1.0, float("nan")),)),
    "infinite sigma": dict(paths=((0, 1.0, float("inf")),)),
    "negative doppler": dict(doppler=-1e-6),
    "doppler above 2^-12": dict(doppler=2.0 ** -12 * (1 + 2.0 ** -50)),
    "nan doppler": dict(doppler=float("nan")),
    "infinite doppler": dict(doppler=float("inf")),
    "33 sinusoids": dict(n_sinusoids=33),
    "negative sinusoids": dict(n_sinusoids=-1),
    "negative first_sample": dict(first_sample=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, _params(g, **BAD[name])) == (-1, False), name
    assert g.lib().dvbt_last_error()
    assert _table(g, _params(g, **BAD[name])) == (-1, True)                    # and nothing is written
    with pytest.raises(g.DvbtError):
        g.fading_table(_params(g, **BAD[name]))


def test_too_many_paths_are_refused(g):
    p = _params(g)
    p.n_paths = 25
    assert _create(g, p) == (-1, False)
    assert _table(g, p) == (-1, True)
    with pytest.raises(ValueError):
        g.FadingParams.of(tuple((i, 1.0, 0.0) for i in range(25)))


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_fading_create.argtypes = [C.POINTER(g.FadingParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_fading_create(None, C.byref(h)) == -1
    assert L.dvbt_fading_create(C.byref(_params(g)), None) == -1
    L.dvbt_fading_table.argtypes = [C.POINTER(g.FadingParams), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    w = (C.c_uint64 * 64)()
    assert L.dvbt_fading_table(None, w, w) == -1
    assert L.dvbt_fading_table(C.byref(_params(g)), None, w) == -1
    assert L.dvbt_fading_table(C.byref(_params(g)), w, None) == -1
    L.dvbt_fading_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.dvbt_fading_run(None, None, 0, None) == -1
    L.dvbt_fading_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert L.dvbt_fading_run_device(None, None, 0, None, None) == -1
    L.dvbt_fading_reset.argtypes = [C.c_void_p]
    assert L.dvbt_fading_reset(None) == -1
    L.dvbt_fading_destroy.argtypes = [C.c_void_p]
    L.dvbt_fading_destroy(None)


@pytest.mark.parametrize("seed", [0, 0xfedcba9876543210])
@pytest.mark.parametrize("doppler", [0.0, 1e-5, 2.0 ** -12])
@pytest.mark.parametrize("npaths", [1, 24])
@pytest.mark.parametrize("M", [1, 16, 32])
def test_the_hosts_table_equals_the_models_word_for_word(g, M, npaths, doppler, seed):
    paths = tuple((i, 0.0, 1.0) for i in range(npaths))
    inc, ph = g.fading_table(_params(g, paths, doppler, M, seed))
    ri, rp = fadingref.table(fadingref.params(paths, doppler, M, seed))
    assert inc.shape == ph.shape == (npaths, M)
    assert [[int(v) for v in row] for row in inc] == ri
    assert [[int(v) for v in row] for row in ph] == rp
    if doppler == 0.0:
        assert not inc.any()
    else:
        assert np.count_nonzero(inc) >= inc.size - 1


def test_zero_sinusoids_are_sixteen(g):
    a = g.fading_table(_params(g, n_sinusoids=0))
    b = g.fading_table(_params(g, n_sinusoids=16))
    assert a[0].shape == (3, 16) and (a[0] == b[0]).all() and (a[1] == b[1]).all()
