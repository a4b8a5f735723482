"""CPU-side checks of the transmit blocks' C ABI (include/dvbt_hip.h, dvbt_txblocks.inc): every entry exported, every params struct laid out as its
ctypes twin in gr_dvbt_amd.binding.BLOCK_PARAMS, and no CPU fallback."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_BLOCKS = ("energy_dispersal", "reed_solomon_enc", "convolutional_interleaver", "inner_coder", "bit_inner_interleaver", "map", "reference_signals")
# make() arguments of a valid configuration (apps/dvbt_tx_demo_8k_QAM64_rate78.grc)
VALID = {
    "energy_dispersal": (4,),
    "reed_solomon_enc": (2, 8, 0x11d, 255, 239, 8, 51, 32),
    "convolutional_interleaver": (544, 12, 17),
    "inner_coder": (1, 6048, 2, 0, 4),
    "bit_inner_interleaver": (6048, 2, 0, 1),
    "map": (6048, 2, 0, 1, 1.0),
    "reference_signals": (8, 6048, 8192, 2, 0, 4, 4, 0, 1, 0, 0),
}


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    gr_dvbt_amd.build()
    return gr_dvbt_amd


def test_block_list_is_the_bindings():
    from gr_dvbt_amd import binding
    assert tuple(binding.TX_BLOCKS) == TX_BLOCKS
    assert all(b in binding.BLOCK_PARAMS for b in TX_BLOCKS)


def test_every_tx_block_entry_is_declared_and_exported(g):
    L = g.lib()
    hdr = open(os.path.join(ROOT, "include", "dvbt_hip.h")).read()
    missing = []
    for b in TX_BLOCKS:
        for fn in ("create", "forecast", "work", "work_device", "destroy"):
            name = f"dvbt_{b}_{fn}"
            if not hasattr(L, name) or f" {name}(" not in hdr:
                missing.append(name)
        if f"}} dvbt_{b}_params;" not in hdr:
            missing.append(f"dvbt_{b}_params")
    assert not missing, missing


def test_params_have_the_headers_layout(g, tmp_path):
    P = g.BLOCK_PARAMS
    lines, want = [], []
    for b in TX_BLOCKS:
        st = P[b]
        lines.append(f'printf("%zu\\n", sizeof(dvbt_{b}_params));')
        want.append(C.sizeof(st))
        for name, _ in st._fields_:
            lines.append(f'printf("%zu\\n", offsetof(dvbt_{b}_params, {name}));')
            want.append(getattr(st, name).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvbt_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


@pytest.mark.parametrize("blk", TX_BLOCKS)
def test_create_has_no_cpu_fallback(g, blk):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = g.lib()
    h = C.c_void_p()
    p = g.BLOCK_PARAMS[blk](*VALID[blk])
    fn = getattr(L, f"dvbt_{blk}_create")
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    assert fn(C.byref(p), C.byref(h)) == -2
    assert not h.value
    with pytest.raises(g.DvbtError):
        g.Block(blk, *VALID[blk])
