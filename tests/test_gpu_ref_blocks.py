"""The per-block GPU entries against what the REFERENCE's own blocks produced, recorded in tests/golden/ref_blocks.json / .npz (make_golden.py --ref-blocks,
from oracle/_ref/libdvbt_blocks_ref.so: the reference's block sources compiled unmodified; tests/test_oracle_ref_blocks.py checks the recordings against it
wherever it is built).  Nothing here reads the reference: every case's input is regenerated from its seed (oracle/ref_cases.py), the GPU block is driven in
the recorded calls with the recorded input tags, and must give the recorded result -- integer outputs by SHA-256, items produced and consumed per call and
the output tags exactly; the demodulator's equalised carriers within the EQ-tap contract |d| <= 1e-3 * 2 * d_norm per component, the mapper's points and
reference_signals' cells within 1e-5 of the peak (no tolerance is new).  The float values compared are the reference's: the few symbols the
recording holds, and the whole output as the oracle gives it once its SHA-256 is the recorded one (the reference's bits).

The hierarchical 64-QAM LP bytes that the reference reads from behind its matrix are excluded (ref_cases.lp_undefined_mask); the Reed-Solomon case runs the
GPU decoder with oracle_compat = 1, which is the reference as compiled.

The driving of a case and every comparison live in tests/refcheck.py, one copy for this module and for tests/test_gpu_gr_shells.py (the GNU Radio block shells
on top of these entries, held to the same recordings)."""
import json
import os

import numpy as np
import pytest

import refcheck
from oracle import ref_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_blocks")


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    return gr_dvbt_amd


@pytest.fixture(scope="module")
def mk(g):
    return refcheck.abi_factory(g, rs_compat=1)                                        # the decoder as the reference is compiled: oracle_compat = 1


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN + ".json")), np.load(GOLDEN + ".npz")


def _names(*kinds):
    return [n for n, c in rc.CASES.items() if c["kind"] in kinds]


@pytest.mark.parametrize("name", _names("sym"))
def test_symbol_interleaver(po, mk, golden, name):
    refcheck.case_sym(po, mk, golden, name)


@pytest.mark.parametrize("name", _names("bitdeint", "bitint"))
def test_bit_interleavers(po, mk, golden, name):
    """the hierarchical cases: both outputs through dvbt_bit_inner_deinterleaver_work_hier, in the recorded calls"""
    refcheck.case_bit(po, mk, golden, name)


@pytest.mark.parametrize("name", _names("vit"))
def test_viterbi_block(po, mk, golden, name):
    refcheck.case_vit(po, mk, golden, name)


@pytest.mark.parametrize("name", _names("convint", "convdeint"))
def test_byte_interleavers(po, mk, golden, name):
    refcheck.case_conv(po, mk, golden, name)


def test_reed_solomon(po, mk, golden):
    for name in ("rs_enc", "rs_dec"):
        refcheck.case_rs(po, mk, golden, name)


@pytest.mark.parametrize("name", _names("disp", "coder"))
def test_dispersal_and_inner_coder(po, mk, golden, name):
    refcheck.case_disp_coder(po, mk, golden, name)


@pytest.mark.parametrize("name", _names("descr"))
def test_descrambler(po, mk, golden, name):
    """in the recorded regime: the smallest call, 4 items visible (output 0 of the recording; output 1 is the reference in larger calls)"""
    refcheck.case_descr(po, mk, golden, name)


@pytest.mark.parametrize("name", _names("demap", "map"))
def test_mapper_and_demapper(po, mk, golden, name):
    refcheck.case_map_demap(po, mk, golden, name)


@pytest.mark.parametrize("name", _names("demod"))
def test_demodulator(po, mk, golden, name):
    refcheck.case_demod(po, mk, golden, name)


@pytest.mark.parametrize("name", _names("refsig"))
def test_pilot_insertion(po, mk, golden, name):
    """reference_signals over the payload the reference block was given: the generator's payload cells in the generator's order (the reference put them where
    the generator had them: the recording is the generator's symbols, bit for bit)"""
    refcheck.case_refsig(po, mk, golden, name)
