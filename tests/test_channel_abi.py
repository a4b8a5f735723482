"""CPU-side checks of the channel block's C ABI (include/dvbt_hip.h, dvbt_channel_*): exported, laid out as the binding says, every parameter checked
before the device is asked for, no CPU fallback."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNEL_SYMBOLS = ("dvbt_channel_create", "dvbt_channel_run", "dvbt_channel_run_device", "dvbt_channel_power", "dvbt_channel_reset", "dvbt_channel_destroy")
FIELDS = ("n_paths", "delay", "amp_re", "amp_im", "cfo", "fft_length", "noise_sigma", "seed", "first_sample", "device")


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _params(g, n_paths=2, delay=(57, 19), cfo=3.37, fft_length=2048, noise_sigma=0.1, seed=5, first_sample=0):
    p = g.ChannelParams()
    p.n_paths = n_paths
    for i, d in enumerate(delay):
        p.delay[i], p.amp_re[i], p.amp_im[i] = d, 0.15, -0.1
    p.cfo, p.fft_length, p.noise_sigma, p.seed, p.first_sample, p.device = cfo, fft_length, noise_sigma, seed, first_sample, 0
    return p


def _create(g, p):
    L = g.lib()
    L.dvbt_channel_create.argtypes = [C.POINTER(g.ChannelParams), C.POINTER(C.c_void_p)]
    L.dvbt_channel_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    r = L.dvbt_channel_create(C.byref(p), C.byref(h))
    if h.value:
        L.dvbt_channel_destroy(h)
    return r, bool(h.value)


def test_every_channel_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in CHANNEL_SYMBOLS if not hasattr(L, n)]
    assert not missing, missing


def test_channel_params_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    fmt = " ".join(["%zu"] * (len(FIELDS) + 3))
    offs = ", ".join(f"offsetof(dvbt_channel_params, {f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dvbt_channel_params), {offs}, (size_t)DVBT_CHANNEL_MAX_PATHS, (size_t)DVBT_CHANNEL_MAX_DELAY); '
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = g.ChannelParams
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] + [g.CHANNEL_MAX_PATHS, g.CHANNEL_MAX_DELAY]
    assert got == want
    assert want[-2:] == [8, 8192]


def test_channel_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _create(g, _params(g)) == (-2, False)
    assert _create(g, _params(g, n_paths=0, delay=(), cfo=0.0, fft_length=0, noise_sigma=0.0)) == (-2, False)
    assert _create(g, _params(g, n_paths=8, delay=(1, 8192, 2, 3, 4, 5, 6, 7), first_sample=2 ** 40 + 3)) == (-2, False)
    with pytest.raises(g.DvbtError) as e:
        g.Channel(echoes=((57, 0.15), (19, -0.1j)), cfo=3.37, fft_length=2048, noise_sigma=0.1, seed=5)
    assert "no CPU fallback" in str(e.value)


BAD = {
    "nine paths": dict(n_paths=9),
    "negative path count": dict(n_paths=-1),
    "delay 0": dict(delay=(57, 0)),
    "delay 8193": dict(delay=(8193, 19)),
    "negative sigma": dict(noise_sigma=-0.1),
    "nan sigma": dict(noise_sigma=float("nan")),
    "infinite sigma": dict(noise_sigma=float("inf")),
    "offset without fft_length": dict(cfo=3.37, fft_length=0),
    "negative first_sample": dict(first_sample=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_params_are_refused_before_the_device_is_asked_for(g, name):
    # -1 with or without a GPU: the checks stand in front of the device
    assert _create(g, _params(g, **BAD[name])) == (-1, False), name
    assert g.lib().dvbt_last_error()


def test_null_arguments_are_refused(g):
    L = g.lib()
    L.dvbt_channel_create.argtypes = [C.POINTER(g.ChannelParams), C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.dvbt_channel_create(None, C.byref(h)) == -1
    assert L.dvbt_channel_create(C.byref(_params(g)), None) == -1
    L.dvbt_channel_run_device.argtypes = [C.c_void_p] * 2 + [C.c_size_t] + [C.c_void_p] * 2
    assert L.dvbt_channel_run_device(None, None, 0, None, None) == -1
    L.dvbt_channel_reset.argtypes = [C.c_void_p]
    assert L.dvbt_channel_reset(None) == -1
    with pytest.raises(ValueError):
        g.Channel(echoes=((1, 0.1),) * 9)
