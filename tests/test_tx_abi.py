"""CPU-side checks of the modulator's C ABI (include/dvbt_hip.h, dvbt_tx_*): exported, laid out as the binding says, no CPU fallback."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_SYMBOLS = ("dvbt_tx_create", "dvbt_tx_samples_for", "dvbt_tx_run", "dvbt_tx_run_device", "dvbt_tx_read_carriers", "dvbt_tx_reset",
              "dvbt_tx_destroy")


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def test_every_tx_symbol_is_exported(g):
    L = g.lib()
    missing = [n for n in TX_SYMBOLS if not hasattr(L, n)]
    assert not missing, missing


def test_tx_params_have_the_headers_layout(g, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dvbt_tx_params), offsetof(dvbt_tx_params, scale), '
                   'offsetof(dvbt_tx_params, max_packets), offsetof(dvbt_tx_params, first_packet), offsetof(dvbt_tx_params, keep_carriers), '
                   'offsetof(dvbt_tx_params, device), offsetof(dvbt_tx_params, cell_id)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = g.TxParams
    want = [C.sizeof(P), P.scale.offset, P.max_packets.offset, P.first_packet.offset, P.keep_carriers.offset, P.device.offset, P.cell_id.offset]
    assert got == want


def test_tx_create_has_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = g.lib()
    h = C.c_void_p()
    p = g.TxParams(g.QAM64, g.NH, g.C7_8, g.G1_32, g.T8k, 0, 0, 0.0022097087, 1024, 0, 0, 0)
    assert L.dvbt_tx_create(C.byref(p), C.byref(h)) == -2
    assert not h.value
    with pytest.raises(g.DvbtError) as e:
        g.Tx(g.QAM16, g.C1_2, g.T2k)
    assert "no CPU fallback" in str(e.value)
