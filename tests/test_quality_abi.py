"""The signal-quality entries at the C boundary, without a GPU: the functions are exported, the report's layout is the ctypes mirror's,
and the layouts of the structures the feature must not touch are what they were before it."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sizeof(dvbt_rx_params), sizeof(dvbt_rx_report), sizeof(dvbt_rx_stream_params) before dvbt_rx_quality existed
SIZES_BEFORE = (104, 160, 136)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def test_quality_entries_are_exported(g):
    L = g.lib()
    for name in ("dvbt_rx_enable_quality", "dvbt_rx_quality", "dvbt_debug_quality_channel", "dvbt_debug_quality_post", "dvbt_debug_quality_time"):
        assert hasattr(L, name), name
    assert g.RxQuality is g.binding.RxQuality
    for name in ("enable_quality", "quality"):
        assert callable(getattr(g.Rx, name))


def test_report_layout_and_untouched_structures(tmp_path):
    import gr_dvbt_amd.binding as b
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dvbt_rx_quality_report), offsetof(dvbt_rx_quality_report, post_bits), '
                   'offsetof(dvbt_rx_quality_report, mer_error), offsetof(dvbt_rx_quality_report, flags), '
                   'sizeof(dvbt_rx_params), sizeof(dvbt_rx_report), sizeof(dvbt_rx_stream_params)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [C.sizeof(b.RxQuality), b.RxQuality.post_bits.offset, b.RxQuality.mer_error.offset, b.RxQuality.flags.offset]
    assert tuple(got[4:]) == SIZES_BEFORE == (C.sizeof(b.RxParams), C.sizeof(b.RxReport), C.sizeof(b.StreamParams))


def test_ratios_of_the_mirror():
    import math
    import gr_dvbt_amd.binding as b
    q = b.RxQuality()
    assert math.isnan(q.mer_db) and math.isnan(q.channel_ber) and math.isnan(q.post_viterbi_ber)
    q.mer_carriers, q.mer_signal, q.mer_error = 10, 100.0, 1.0
    q.channel_bits, q.channel_bit_errors, q.post_bits, q.post_bit_errors = 1000, 10, 1504, 0
    assert abs(q.mer_db - 20.0) < 1e-12 and q.channel_ber == 0.01 and q.post_viterbi_ber == 0.0


def test_hooks_refuse_bad_sizes_before_they_ask_for_a_device(g):
    L = g.lib()
    L.dvbt_debug_quality_channel.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dvbt_debug_quality_post.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    buf = (C.c_ubyte * 256)()
    a, e = C.c_int64(), C.c_int64()
    assert L.dvbt_debug_quality_channel(1, 0, buf, -1, buf, 8, C.byref(a), C.byref(e)) == -1
    assert L.dvbt_debug_quality_channel(7, 0, buf, 8, buf, 8, C.byref(a), C.byref(e)) == -1
    assert L.dvbt_debug_quality_channel(1, 0, None, 8, buf, 8, C.byref(a), C.byref(e)) == -1
    assert L.dvbt_debug_quality_post(buf, 204, buf, -1, C.byref(a), C.byref(e)) == -1
    assert L.dvbt_debug_quality_post(buf, (1 << 30) + 1, buf, 1, C.byref(a), C.byref(e)) == -1
    L.dvbt_rx_quality.argtypes = [C.c_void_p, C.c_void_p]
    L.dvbt_rx_enable_quality.argtypes = [C.c_void_p, C.c_int]
    assert L.dvbt_rx_quality(None, None) == -1 and L.dvbt_rx_enable_quality(None, 1) == -1
    if g.device_count() <= 0:     # there is no CPU path
        assert L.dvbt_debug_quality_channel(1, 0, buf, 8, buf, 8, C.byref(a), C.byref(e)) == -2
        assert L.dvbt_debug_quality_post(buf, 204, buf, 1, C.byref(a), C.byref(e)) == -2
