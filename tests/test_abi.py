"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, exports every
symbol include/dvbt_hip.h declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def _declared():
    txt = open(os.path.join(ROOT, "include", "dvbt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dvbt_[a-z0-9_]+)\s*\(", txt)))


def test_every_declared_symbol_is_exported(g):
    L = g.lib()
    names = _declared()
    assert len(names) >= 50
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_one_triple_per_reference_block(g):
    names = set(_declared())
    for blk in ("ofdm_sym_acquisition", "fft", "demod_reference_signals", "demap", "symbol_inner_interleaver",
                "bit_inner_deinterleaver", "viterbi_decoder", "convolutional_deinterleaver", "reed_solomon_dec",
                "energy_descramble"):
        for fn in ("create", "forecast", "work", "destroy"):
            assert f"dvbt_{blk}_{fn}" in names


def test_dims_match_reference_table(g):
    # SURVEY Appendix A
    d = g.get_dims(g.QAM64, g.C7_8, g.T8k)
    assert (d.fft_length, d.cp_length, d.Kmax, d.payload_length, d.zeros_on_left, d.m, d.cr_k, d.cr_n, d.ntraceback) == \
        (8192, 256, 6816, 6048, 688, 6, 7, 8, 24)
    assert d.info_bits_per_symbol == 3969 * 8
    d = g.get_dims(g.QAM16, g.C1_2, g.T2k)
    assert (d.fft_length, d.cp_length, d.payload_length, d.zeros_on_left, d.m, d.ntraceback) == (2048, 64, 1512, 172, 4, 5)
    assert d.info_bits_per_symbol == 378 * 8
    with pytest.raises(g.DvbtError):
        g.get_dims(7, 0, 0)


def test_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(g.DvbtError) as e:
        g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=1 << 20)
    assert "no CPU fallback" in str(e.value)
    L = g.lib()
    h = C.c_void_p()

    class P(C.Structure):
        _fields_ = [("fft_size", C.c_int), ("forward", C.c_int), ("shift", C.c_int)]
    assert L.dvbt_fft_create(C.byref(P(2048, 1, 1)), C.byref(h)) == -2
    # the test hooks that launch kernels: bad sizes are refused first, then the missing device; a hook on a handle says so before it asks for the handle
    rep = (C.c_int64 * 16)()
    buf = (C.c_ubyte * 204)()
    L.dvbt_debug_outer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_debug_outer_read.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_size_t]
    L.dvbt_debug_outer_read.restype = C.c_int64
    assert L.dvbt_debug_outer(None, 0, buf, -1, 0, 0, rep, None, 0) == -1
    assert L.dvbt_debug_outer(None, 0, buf, (1 << 30) + 1, 0, 0, rep, None, 0) == -1
    for mode in (0, 1, 2):
        assert L.dvbt_debug_outer(None, mode, buf, 204, 0, 0, rep, None, 0) == -2
    assert L.dvbt_debug_outer_read(None, 1, 0, buf, 8) == -2
    # dvbt_debug_drift: null pointers, a negative nsym, more calls than its scratch is sized for, an unknown path, an N / cp that is no mode / guard pair
    L.dvbt_debug_drift.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    sw, inc, ph, fl, delta = (C.c_int32 * 4)(), (C.c_double * 4)(), (C.c_float * 4)(), (C.c_int32 * 4)(), (C.c_float * (4 * 256))()
    ok = [8192, 256, 4, sw, inc, inc, ph, 0, 0, delta, fl, None]
    for i, v in ((3, None), (4, None), (5, None), (6, None), (9, None), (10, None), (2, -1), (2, 65537), (8, 2), (8, -1),
                 (0, 4096), (0, 0), (1, 0), (1, 255), (1, 4096), (1, 128)):
        bad = list(ok)
        bad[i] = v
        assert L.dvbt_debug_drift(*bad) == -1, (i, v)
    for N, cp, path in ((8192, 256, 0), (8192, 2048, 1), (2048, 64, 0), (2048, 512, 1), (2048, 128, 0), (8192, 1024, 0)):
        assert L.dvbt_debug_drift(N, cp, 4, sw, inc, inc, ph, 0, path, delta, fl, None) == -2
    # dvbt_debug_symbols: what it can refuse without a handle (null pointers, nsym < 1, a negative grid, avail outside (0, nsamples], a negative call0 or nread, non-finite
    # phases) before it asks for the device; the refusals that need the handle's sizes are in tests/test_gpu_symbol_kernels.py
    L.dvbt_debug_symbols.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    iq, cps, phs = (C.c_float * (2 * 4096))(), (C.c_int32 * 4)(), (C.c_float * 4)()
    nan_f, inf_d = (C.c_float * 4)(0, float("nan"), 0, 0), (C.c_double * 4)(0, 0, 0, float("inf"))
    ok = [None, iq, 4096, 4, 0, 1, 4096, cps, sw, phs, inc, inc, 0, None, 0] + [None] * 8
    for i, v in ((1, None), (7, None), (8, None), (9, None), (10, None), (11, None), (3, 0), (3, -2), (12, -1), (6, 0), (6, -1), (6, 4097), (2, 0), (4, -1), (14, -1),
                 (9, nan_f), (10, inf_d), (11, inf_d)):
        bad = list(ok)
        bad[i] = v
        assert L.dvbt_debug_symbols(*bad) == -1, (i, v)
    assert L.dvbt_debug_symbols(*ok) == -2
    # dvbt_debug_frames: null pointers, a negative n_symbols, a sym_off that is negative or no multiple of 272, a start_delay_symbols outside [0, 272) before it asks
    # for the device; the refusals that need the handle (null, soft decisions, n_symbols beyond its calls) are in tests/test_gpu_frames.py
    L.dvbt_debug_frames.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_int] + [C.c_void_p] * 7
    i32, tps, lab, frep, st = (C.c_int32 * 8)(), (C.c_float * (2 * 8 * 68))(), (C.c_ubyte * (8 * 6048))(), (C.c_int64 * 32)(), (C.c_int64 * 4)()
    ok = [None, 8, 1, i32, tps, None, None, lab, 0, 0, frep, i32, i32, st, lab, None, None]
    for i, v in ((3, None), (4, None), (7, None), (10, None), (11, None), (12, None), (13, None), (14, None), (1, -1), (8, 1), (8, 271), (8, -272), (9, -1), (9, 272)):
        bad = list(ok)
        bad[i] = v
        assert L.dvbt_debug_frames(*bad) == -1, (i, v)
    assert L.dvbt_debug_frames(*ok) == -2
    assert all(x == 0 for x in frep) and all(x == 0 for x in st)
    # dvbt_debug_acquire: null pointers, sizes, an unknown path or force before it asks for the device; what needs the handle is in tests/test_gpu_acquire.py
    L.dvbt_debug_acquire.argtypes = g.binding.ACQUIRE_ARGTYPES
    ok = [None, iq, 4096, 0, 4096, 4, 0, 0.0, 0, 0, C.byref(g.binding.AcquireReport()), lab, 4] + [None] * 7
    for i, v in ((1, None), (10, None), (11, None), (2, 0), (3, -1), (4, 0), (4, 4097), (5, 0), (5, 65), (8, 2), (9, 3), (12, -1)):
        bad = list(ok)
        bad[i] = v
        assert L.dvbt_debug_acquire(*bad) == -1, (i, v)
    assert L.dvbt_debug_acquire(*ok) == -2


def test_viterbi_block_test_hooks_refuse_without_a_device(g):
    """dvbt_viterbi_decoder_set_chunk_bytes / _set_verify / _last_ctl: a value out of range is refused before the handle is looked at, a null handle after it"""
    L = g.lib()
    L.dvbt_last_error.restype = C.c_char_p
    for fn in (L.dvbt_viterbi_decoder_set_chunk_bytes, L.dvbt_viterbi_decoder_set_verify):
        fn.argtypes = [C.c_void_p, C.c_int]
    L.dvbt_viterbi_decoder_last_ctl.argtypes = [C.c_void_p, C.c_void_p]
    fake = C.c_void_p(1)                                                    # never dereferenced: the value is refused first
    for bad in (23, 25, 288, -24):
        for h in (None, fake):
            assert L.dvbt_viterbi_decoder_set_chunk_bytes(h, bad) == -1 and b"multiple of 24 in [24, 264]" in L.dvbt_last_error(), bad
    for bad in (-2, 5):
        for h in (None, fake):
            assert L.dvbt_viterbi_decoder_set_verify(h, bad) == -1 and b"[-1, 4]" in L.dvbt_last_error(), bad
    for ok in (0, 24, 48, 264):
        assert L.dvbt_viterbi_decoder_set_chunk_bytes(None, ok) == -1 and b"null handle" in L.dvbt_last_error(), ok
    for ok in (-1, 0, 1, 2, 3, 4):
        assert L.dvbt_viterbi_decoder_set_verify(None, ok) == -1 and b"null handle" in L.dvbt_last_error(), ok
    out = (C.c_int * 16)()
    assert L.dvbt_viterbi_decoder_last_ctl(None, out) == -1 and L.dvbt_viterbi_decoder_last_ctl(None, None) == -1


def test_product_does_not_import_oracle():
    """The product path must not route through the oracle (or any CPU fallback)."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gr_dvbt_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".inc", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "pyoracle" not in txt and "dvbt_oracle.h" not in txt and "liboracle" not in txt, os.path.join(dirpath, f)


def test_ctypes_structures_have_the_headers_layout(tmp_path):
    """the structures of gr_dvbt_amd/binding.py against include/dvbt_hip.h as a C compiler lays them out (sizes, the offsets of the newest fields): a field added on one
    side only would shift everything behind it silently"""
    import ctypes as C
    import subprocess
    import gr_dvbt_amd.binding as b
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dvbt_rx_params), offsetof(dvbt_rx_params, viterbi_warm_windows), '
                   'offsetof(dvbt_rx_params, max_samples), sizeof(dvbt_rx_stream_params), offsetof(dvbt_rx_stream_params, segment_superframes), '
                   'offsetof(dvbt_rx_stream_params, borrow_device_pushes), sizeof(dvbt_rx_report)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(b.RxParams), b.RxParams.viterbi_warm_windows.offset, b.RxParams.max_samples.offset, C.sizeof(b.StreamParams),
            b.StreamParams.segment_superframes.offset, b.StreamParams.borrow_device_pushes.offset, C.sizeof(b.RxReport)]
    assert got == want
