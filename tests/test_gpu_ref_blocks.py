"""The per-block GPU entries against what the REFERENCE's own blocks produced, recorded in tests/golden/ref_blocks.json / .npz (make_golden.py --ref-blocks,
from oracle/_ref/libdvbt_blocks_ref.so: the reference's block sources compiled unmodified; tests/test_oracle_ref_blocks.py checks the recordings against it
wherever it is built).  Nothing here reads the reference: every case's input is regenerated from its seed (oracle/ref_cases.py), the GPU block is driven in
the recorded calls with the recorded input tags, and must give the recorded result -- integer outputs by SHA-256, items produced and consumed per call and
the output tags exactly; the demodulator's equalised carriers within the EQ-tap contract |d| <= 1e-3 * 2 * d_norm per component, the mapper's points and
reference_signals' cells within 1e-5 of the peak (no tolerance is new).  The float values compared are the reference's: the few symbols the
recording holds, and the whole output as the oracle gives it once its SHA-256 is the recorded one (the reference's bits).

The hierarchical 64-QAM LP bytes that the reference reads from behind its matrix are excluded (ref_cases.lp_undefined_mask); the Reed-Solomon case runs the
GPU decoder with oracle_compat = 1, which is the reference as compiled."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import ref_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_blocks")
KEYS = {"sync_start": 1, "superframe_start": 2, "symbol_index": 3}
NAMES = {v: k for k, v in KEYS.items()}


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    return gr_dvbt_amd


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN + ".json")), np.load(GOLDEN + ".npz")


def _names(*kinds):
    return [n for n, c in rc.CASES.items() if c["kind"] in kinds]


def _drive(b, x, in_item, out_item, calls, in_tags=(), visible=None):
    """the recorded calls [noutput, returned, consumed] on the GPU block: every call sees `visible(noutput)` input items from where the last one stopped and the
    input tags that fall among them; returns (output bytes, [[noutput, returned, consumed]], [[0, absolute offset, key, value]])"""
    x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    total = len(x) // in_item
    pos, written, outs, log, tags = 0, 0, [], [], []
    for n, _, _ in calls:
        vis = min(visible(n) if visible else b.forecast(n), total - pos)
        tin = [(t - pos, KEYS[k], v) for t, k, v in in_tags if pos <= t < pos + vis]
        out = np.zeros(n * out_item, np.uint8)
        r, cons, tout = b.work(n, vis, x[pos * in_item:(pos + vis) * in_item], out, tin)
        log.append([n, r, cons])
        tags += [[0, written + off, NAMES[key], val] for off, key, val in tout]
        outs.append(out[:r * out_item])
        pos += cons
        written += r
    b.close()
    return (np.concatenate(outs) if outs else np.zeros(0, np.uint8)), log, tags


def _check(want, out, log, tags, port=0):
    assert log == rc.unrle(want["log"])
    assert tags == rc.unrle(want["tags"])
    assert len(out) == want["nbytes"][port] and rc.sha(out) == want["sha256"][port]


@pytest.mark.parametrize("name", _names("sym"))
def test_symbol_interleaver(po, g, golden, name):
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    P = rc.P8K if case["mode"] else rc.P2K
    b = g.Block("symbol_inner_interleaver", P, case["mode"], case["direction"])
    tags = [(i, "symbol_index", s) for i, s in enumerate(case["indices"])]
    _check(want, *_drive(b, inp["in"][0], P, P, rc.unrle(want["log"]), tags))


@pytest.mark.parametrize("name", _names("bitdeint", "bitint"))
def test_bit_interleavers(po, g, golden, name):
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    x = inp["in"][0]
    calls = rc.unrle(want["log"])
    if case["kind"] == "bitint" or case["hier"] == 0:
        b = g.Block("bit_inner_interleaver" if case["kind"] == "bitint" else "bit_inner_deinterleaver", rc.P2K, case["const"], 0, 0)
        _check(want, *_drive(b, x, rc.P2K, rc.P2K, calls))
        return
    L = g.lib()
    L.dvbt_bit_inner_deinterleaver_work_hier.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    b = g.Block("bit_inner_deinterleaver", rc.P2K, case["const"], case["hier"], 0)
    pos, oh, ol = 0, [], []
    for n, r, cons in calls:                                                           # both outputs, in the recorded calls
        h, lo = np.zeros(n * rc.P2K, np.uint8), np.full(n * rc.P2K, 0xee, np.uint8)
        xi = np.ascontiguousarray(x[pos * rc.P2K:(pos + n) * rc.P2K])
        assert L.dvbt_bit_inner_deinterleaver_work_hier(b.h, n, n, xi.ctypes.data, h.ctypes.data, lo.ctypes.data, None) == r
        oh.append(h)
        ol.append(lo)
        pos += cons
    b.close()
    oh, ol = np.concatenate(oh), rc._mask_lp(case, np.concatenate(ol))
    assert len(oh) == want["nbytes"][0] and rc.sha(oh) == want["sha256"][0]
    assert len(ol) == want["nbytes"][1] and rc.sha(ol) == want["sha256"][1]


@pytest.mark.parametrize("name", _names("vit"))
def test_viterbi_block(po, g, golden, name):
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    b = g.Block("viterbi_decoder", case["const"], 0, case["rate"], 768, 0, -1)
    tags = [(t, "superframe_start", 0xaa) for t in inp["tags"]]
    _check(want, *_drive(b, inp["in"][0], 1, 1, rc.unrle(want["log"]), tags))


@pytest.mark.parametrize("name", _names("convint", "convdeint"))
def test_byte_interleavers(po, g, golden, name):
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    if case["kind"] == "convint":
        b = g.Block("convolutional_interleaver", 136, 12, 17)
        _check(want, *_drive(b, inp["in"][0], 1632, 1, rc.unrle(want["log"])))
    else:
        b = g.Block("convolutional_deinterleaver", 136, 12, 17)
        tags = [(t, "superframe_start", 1) for t in case["tags"]]
        _check(want, *_drive(b, inp["in"][0], 1, 1632, rc.unrle(want["log"]), tags))


def test_reed_solomon(po, g, golden):
    for name, blk, sizes in (("rs_enc", "reed_solomon_enc", (8 * 188, 8 * 204)), ("rs_dec", "reed_solomon_dec", (8 * 204, 8 * 188))):
        case, want = rc.CASES[name], golden[0]["cases"][name]
        inp = rc.make_input(po, case)
        b = g.Block(blk, *(rc.RS_ARGS + ([1] if blk == "reed_solomon_dec" else [])))    # the decoder as the reference is compiled: oracle_compat = 1
        _check(want, *_drive(b, inp["in"][0], sizes[0], sizes[1], rc.unrle(want["log"])))


@pytest.mark.parametrize("name", _names("disp", "coder"))
def test_dispersal_and_inner_coder(po, g, golden, name):
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    if case["kind"] == "disp":
        # every byte that is left is visible: behind a sync byte at offset i the reference reads i + 1504 bytes whatever ninput_items says (its forecast
        # promises 1512), the GPU block takes an item only when it has been given all of it
        b = g.Block("energy_dispersal", 1)
        _check(want, *_drive(b, inp["in"][0], 1, 1504, rc.unrle(want["log"]), visible=lambda n: 1 << 30))
    else:
        b = g.Block("inner_coder", 1, rc.P2K, case["const"], case["hier"], case["rate"])
        _check(want, *_drive(b, inp["in"][0], 1, rc.P2K, rc.unrle(want["log"])))


@pytest.mark.parametrize("name", _names("descr"))
def test_descrambler(po, g, golden, name):
    """in the recorded regime: the smallest call, 4 items visible (output 0 of the recording; output 1 is the reference in larger calls)"""
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    b = g.Block("energy_descramble", 8)
    _check(want, *_drive(b, inp["in"][0], 1504, 1, rc.unrle(want["log"]), visible=lambda n: 4))


@pytest.mark.parametrize("name", _names("demap", "map"))
def test_mapper_and_demapper(po, g, golden, name):
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    calls = rc.unrle(want["log"])
    if case["kind"] == "demap":
        b = g.Block("demap", rc.P2K, case["const"], case["hier"], 0, 1.0)
        _check(want, *_drive(b, inp["in"][0], 8 * rc.P2K, rc.P2K, calls))
        return
    b = g.Block("map", rc.P2K, case["const"], case["hier"], 0, 1.0)
    out, log, tags = _drive(b, inp["in"][0], rc.P2K, 8 * rc.P2K, calls)
    assert log == calls and tags == [] and len(out) == want["nbytes"][0]
    got = out.view(np.complex64)
    ref = rc.run_oracle(po, case, inp)["out"][0]
    assert rc.sha(ref) == want["sha256"][0]                                            # the oracle's points are the reference's, bit for bit
    for key, (off, nbytes) in want["kept"].items():
        kept = golden[1][key]
        assert (ref[off:off + nbytes].view(np.complex64) == kept).all()
        assert np.abs(got[off // 8:(off + nbytes) // 8] - kept).max() <= 1e-5 * np.abs(kept).max()
    ref = ref.view(np.complex64)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize("name", _names("demod"))
def test_demodulator(po, g, golden, name):
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    c = inp["cfg"]
    b = g.Block("demod_reference_signals", 8, c.N, c.payload, case["const"], 0, case["rate"], case["rate"], 0, case["mode"], 0, 0)
    tags = [(t, "sync_start", 1) for t in case["sync"]]
    out, log, otags = _drive(b, inp["in"][0], 8 * c.N, 8 * c.payload, rc.unrle(want["log"]), tags, visible=lambda n: 2 * n)
    assert log == rc.unrle(want["log"])
    assert otags == rc.unrle(want["tags"])
    assert len(out) == want["nbytes"][0] > 0
    got = out.view(np.complex64)
    tol = 1e-3 * 2 * c.norm                                                            # the EQ-tap contract, DESIGN 7
    for key, (off, nbytes) in want.get("kept", {}).items():                            # the reference's recorded values
        d = got[off // 8:(off + nbytes) // 8] - golden[1][key]
        assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= tol
    ref = rc.run_oracle(po, case, inp)["out"][0]
    assert rc.sha(ref) == want["sha256"][0]                                            # the reference's bits, all items
    d = got - ref.view(np.complex64)
    assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= tol


@pytest.mark.parametrize("name", _names("refsig"))
def test_pilot_insertion(po, g, golden, name):
    """reference_signals over the payload the reference block was given: the generator's payload cells in the generator's order (the reference put them where
    the generator had them: the recording is the generator's symbols, bit for bit)"""
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    c = inp["cfg"]
    F = inp["F"]
    assert rc.sha(np.ascontiguousarray(F[:want["nbytes"][0] // (8 * c.N)]).reshape(-1).view(np.uint8)) == want["sha256"][0]
    # payload cells of a symbol: every carrier that is no pilot and no TPS cell, in rising order -- read off a run of the block itself over numbered cells
    cell = case.get("cell", (0, 0))
    args = (8, c.payload, c.N, case["const"], 0, case["rate"], case["rate"], 0, case["mode"], cell[0], cell[1])
    n = inp["nitems"]
    mark = np.zeros((n, c.payload), np.complex64)
    mark.real = 1000 + np.arange(c.payload)
    mark.imag = 7
    numbered, _, _ = _drive(g.Block("reference_signals", *args), mark, 8 * c.payload, 8 * c.N, [[n, n, n]])
    numbered = numbered.view(np.complex64).reshape(n, c.N)
    pos = np.stack([np.flatnonzero(numbered[s].imag == 7) for s in range(n)])
    assert pos.shape == (n, c.payload)
    pay = np.take_along_axis(F, pos, axis=1)
    out, log, tags = _drive(g.Block("reference_signals", *args), pay, 8 * c.payload, 8 * c.N, rc.unrle(want["log"]))
    assert log == rc.unrle(want["log"]) and tags == [] and len(out) == want["nbytes"][0]
    got = out.view(np.complex64)
    ref = np.ascontiguousarray(F[:len(got) // c.N]).reshape(-1)
    peak = np.abs(ref).max()
    for key, (off, nbytes) in want.get("kept", {}).items():
        assert np.abs(got[off // 8:(off + nbytes) // 8] - golden[1][key]).max() <= 1e-5 * peak
    assert np.abs(got - ref).max() <= 1e-5 * peak
