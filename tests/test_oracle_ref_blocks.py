"""Pin the oracle's stages against the REFERENCE's own blocks, executed.

oracle/_ref/libdvbt_blocks_ref.so is the reference's lib/<block>_impl.cc, dvbt_config.cc, reed_solomon.cc and d_*.c compiled unmodified against the stand-in
headers of oracle/ref_standin/ and driven by oracle/ref_driver.cc (oracle/Makefile target `ref`): the block is made through its own make(), its general_work /
work runs on our buffers, item counts and input tags, and what comes back is the items produced, the items consumed and the output tags.  The cases, their
seeded inputs and the oracle's side of each comparison are in oracle/ref_cases.py.

Where the library is built, every case runs the reference block and the oracle's stage function in the same calls and compares outputs BIT FOR BIT (the
float outputs -- equalised carriers, mapper points, the pilot / TPS cells -- as float bits: none differs, so no tolerance exists in this module), the
per-call counts and the output tags; the recordings of tests/golden/ref_blocks.json (make_golden.py --ref-blocks) are checked against the reference in the
same run.  Where it is not built, the oracle is compared with the recordings.

Stated deviations: the bytes of the hierarchical 64-QAM LP stream that the reference reads from behind its bit matrix are excluded
(ref_cases.lp_undefined_mask: words i >= 84, every second one, of a 126-word block); the as-compiled reference's Reed-Solomon decoder is the oracle's
compat mode (SURVEY B-1); energy_descramble's output depends on the call pattern once a sync byte is damaged (test_descrambler_call_pattern).
"""
import json
import os

import numpy as np
import pytest

from oracle import ref_cases as rc
from oracle import refblocks as rb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_blocks")
LIVE = rb.available()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN + ".json")), np.load(GOLDEN + ".npz")


def _same(a, b, what):
    assert len(a) == len(b), "%s: %d bytes against %d" % (what, len(a), len(b))
    d = np.flatnonzero(a != b)
    assert len(d) == 0, "%s: %d bytes differ, the first at %d" % (what, len(d), d[0])


def check_case(po, golden, name):
    """oracle == reference (live) == recording; returns (case, input, oracle's run, reference's run or None)"""
    case = rc.CASES[name]
    meta, floats = golden
    want = meta["cases"][name]
    inp = rc.make_input(po, case)
    ora = rc.run_oracle(po, case, inp)
    ref = None
    if LIVE:
        ref = rc.run_ref(case, inp)
        assert rc.record(ref) == {k: v for k, v in want.items() if k not in ("kept", "sched")}, "the recording is not what the reference block produces"
        # what the block asks of the scheduler -- output multiple, relative rate, item sizes, forecast at every noutput_items of its calls -- as recorded for
        # tests/test_gpu_gr_shells.py (the project's GNU Radio shells are held to it there)
        assert rc.sched(ref) == want["sched"], "the recorded scheduler hints are not the reference block's"
        for j, o in enumerate(ora["out"]):
            _same(o, ref["out"][j], "%s output %d, oracle against reference" % (name, j))
        for key in ("log", "tags"):
            if ora[key] is not None:
                assert ora[key] == ref[key], "%s %s" % (name, key)
    for j, o in enumerate(ora["out"]):
        assert len(o) == want["nbytes"][j] and rc.sha(o) == want["sha256"][j], "%s output %d against the recording" % (name, j)
    for key in ("log", "tags"):
        if ora[key] is not None:
            assert ora[key] == rc.unrle(want[key]), "%s %s against the recording" % (name, key)
    for key in want.get("kept", ()):                                                   # the float values kept for tests/test_gpu_ref_blocks.py
        off, nbytes = want["kept"][key]
        src = ref if ref is not None else ora
        _same(src["out"][0][off:off + nbytes], floats[key].view(np.uint8).reshape(-1), "%s kept values at byte %d" % (name, off))
    return case, inp, ora, ref


def _names(*kinds):
    return [n for n, c in rc.CASES.items() if c["kind"] in kinds]


def test_every_case_is_recorded(golden):
    assert sorted(golden[0]["cases"]) == sorted(rc.CASES)
    for name, want in golden[0]["cases"].items():                                      # ... with its scheduler hints, forecast at every call size of its log
        for h in want["sched"] if isinstance(want["sched"], list) else [want["sched"]]:
            assert sorted(h) == ["forecast", "in_itemsize", "out_itemsize", "output_multiple", "relative_rate"], name
        if rc.CASES[name]["kind"] != "chain":
            sizes = {e[0] for key in ("log", "log_big") for e in rc.unrle(want.get(key, []))}
            assert {f[0] for f in want["sched"]["forecast"]} == sizes, name


@pytest.mark.parametrize("name", _names("sym"))
def test_symbol_interleaver(po, golden, name):
    """o_sym_H / o_sym_interleave against symbol_inner_interleaver, both directions, 2k and 8k: the de-interleaver takes every item's parity from its
    symbol_index tag (a repeated and a skipped index among them: parity stops alternating), the interleaver counts for itself; calls of 1 and 3 items"""
    case, inp, ora, _ = check_case(po, golden, name)
    assert len(ora["out"][0]) >= 9 * (rc.P8K if case["mode"] else rc.P2K)


@pytest.mark.parametrize("name", _names("bitdeint", "bitint"))
def test_bit_interleavers(po, golden, name):
    """o_bit_deinterleave / o_bit_deinterleave_hier (both outputs) / o_bit_interleave against the blocks: random labels, every single bit position alone, all
    bits set.  Hierarchical QPSK is not constructed (the reference divides by zero); the hierarchical interleaver is not constructed either: it WRITES behind
    its matrix for 64-QAM."""
    case, inp, ora, _ = check_case(po, golden, name)
    if case["kind"] == "bitdeint" and case["hier"] and case["const"] == 2:
        m = rc.lp_undefined_mask()
        assert list(np.flatnonzero(m)) == list(range(84, 126, 2))                       # row 5, words i >= 84: DESIGN 7
        assert ora["out"][1].any()


@pytest.mark.parametrize("name", _names("vit"))
def test_viterbi_block(po, golden, name):
    """o_viterbi_decode_n, period by period as oracle/o_chain.c lays the periods out, against the viterbi_decoder BLOCK: its depuncturer, its output cadence
    (the first call of a period returns ntraceback bytes less), its superframe_start tag in and out, and what it drops in front of a tag.  The bytes are
    o_viterbi_decode_n's; the layout of the calls around a tag is ref_cases.py's own model of the block (the oracle's C for it, o_chain.c, is run by
    test_receive_chain)"""
    case, inp, ora, _ = check_case(po, golden, name)
    if case["ber"] == 0.0 and len(case["tag_blocks"]) == 1:
        n = len(ora["out"][0])
        assert n > 0 and (ora["out"][0] == inp["data"][:n]).all()                       # and it decodes what was encoded
    if len(case["tag_blocks"]) > 1:
        assert len(ora["tags"]) == 2                                                    # the re-tag
        if "inside" in name:
            assert any(e[1] == 0 and e[2] > 0 for e in ora["log"])                      # the call that drops what lies in front of the tag


@pytest.mark.parametrize("name", _names("convint", "convdeint"))
def test_byte_interleavers(po, golden, name):
    """o_conv_interleave / o_conv_deinterleave against the blocks, 24 to 60 RS words, output in pairs of items; a superframe_start tag at item 0 changes nothing,
    one further in makes the de-interleaver drop what lies in front of it -- and keep its FIFOs.  The bytes are o_conv_*'s; how much is taken in
    front of a tag is o_conv_deint_taken_before_tag's (o_chain.c's rule) in the cases that call for one pair at a time, ref_cases.py's own model of the block otherwise"""
    case, inp, ora, _ = check_case(po, golden, name)
    if case["kind"] == "convdeint":
        assert all(e[0] % 2 == 0 for e in ora["log"])
        if max(case["tags"]) > 0:
            assert [e[1:] for e in ora["log"] if e[1] == 0]


def test_rs_encoder(po, golden):
    check_case(po, golden, "rs_enc")


def test_rs_decoder(po, golden):
    """the as-compiled reference decoder IS o_rs_decode's compat mode, exactly (SURVEY B-1): 0, 1, 8 and 9 symbol errors, at the first, the last and the
    parity positions, the all-zero word.  The default mode differs from it only as B-1 says: in a word that is corrected, the correction at the lowest
    error location is not made (it lands in front of the word)."""
    case, inp, ora, _ = check_case(po, golden, "rs_dec")
    compat = ora["out"][0].reshape(-1, 188)
    good = rc.rs_decode(po, inp["in"][0], len(compat), 0).reshape(-1, 188)
    recv = inp["in"][0].reshape(-1, 204)
    ndiffer = 0
    for i, pos in enumerate(inp["errpos"]):
        d = list(np.flatnonzero(good[i] != compat[i]))
        if len(pos) <= 8:
            assert (good[i] == inp["sent"][i, :188]).all()                              # the textbook decoder corrects up to 8
            first = pos[0] if pos else None
            assert d == ([first] if first is not None and first < 188 else []), (i, pos, d)
            if d:
                assert compat[i, first] == recv[i, first]                               # left as received
                ndiffer += 1
        else:
            assert d == [] and (good[i] == recv[i, :188]).all()                         # beyond the code: both pass the word on
    assert ndiffer >= 6


@pytest.mark.parametrize("name", _names("disp", "coder"))
def test_dispersal_and_inner_coder(po, golden, name):
    """o_energy_dispersal (a TS that starts on its sync byte, and one behind 77 other bytes) and the TX path's inner coder (o_inner_code: every rate and
    constellation, and one hierarchical mode) against the blocks"""
    check_case(po, golden, name)


@pytest.mark.parametrize("name", _names("descr"))
def test_descrambler(po, golden, name):
    """o_energy_descramble against energy_descramble in the regime oracle/o_chain.c states (4 items visible, 2 consumed): streams that start at each of the 8
    packet phases, a damaged inverted sync byte, a stretch with sync lost and regained; o_energy_descramble_groups from the first NSYNC on gives the same bytes on
    the undamaged streams"""
    import ctypes as C
    case, inp, ora, _ = check_case(po, golden, name)
    if case["damage"] == "none":
        out = ora["out"][0]
        first = ((8 - case["phase"]) % 8) * 188
        o = np.zeros(len(out), np.uint8)
        L = po.lib()
        L.o_energy_descramble_groups.restype = C.c_size_t
        x = np.ascontiguousarray(inp["in"][0][first:])
        n = L.o_energy_descramble_groups(x.ctypes.data_as(C.c_void_p), C.c_size_t(len(out) // 1504), o.ctypes.data_as(C.c_void_p))
        assert n == len(out) > 0 and (o == out).all()


def test_descrambler_call_pattern(golden):
    """What was found by driving the reference in larger calls as well (12 items visible, 10 consumed): the block looks at ONE byte per call, the one at its
    offset, so on an undamaged stream the output does not depend on the call pattern; a damaged inverted sync byte is noticed only where a call starts on it,
    and a lost sync only at the next call's start: there the output depends on the pattern (the larger calls descramble the damaged stretch through).
    Also: forecast asks for 4 items per item of output (16 for the smallest call) although no call reads beyond 4: a scheduler holds back more at the end of
    a stream than the oracle's regime does, nothing else changes."""
    cases = golden[0]["cases"]
    for phase in range(8):
        assert cases["descr_phase%d" % phase]["big_equals_small"] is True
    assert cases["descr_bad_nsync_inside_call"]["big_equals_small"] is True
    assert cases["descr_bad_nsync_at_call_start"]["big_equals_small"] is False
    assert cases["descr_sync_lost"]["big_equals_small"] is False
    assert [e[1] for e in rc.unrle(cases["descr_sync_lost"]["log"])].count(0) == 2                # two calls that find no NSYNC and drop two items each
    if LIVE:
        assert rb.Block("energy_descramble", [1]).forecast(4 * 1504) == [16]


@pytest.mark.parametrize("name", _names("demap", "map"))
def test_mapper_and_demapper(po, golden, name):
    """o_constellation + o_demap against dvbt_demap (labels exact) and dvbt_map (float bits), alpha 1 / 2 / 4: every point, every midpoint between neighbours
    and every four-way tie, the floats next to every decision boundary, the centre gap, points far outside, noisy points"""
    case, inp, ora, _ = check_case(po, golden, name)
    if case["kind"] == "demap":
        c = rc._cfg(po, case)
        assert (ora["out"][0][:c.csize] == np.arange(c.csize)).all()                    # the points themselves
        assert len(np.unique(ora["out"][0])) == c.csize


@pytest.mark.parametrize("name", _names("demod"))
def test_demodulator(po, golden, name):
    """o_demod_work against demod_reference_signals, one item per call: items produced and consumed, the symbol_index and superframe_start tags (the TPS state
    machine seen through them) and the equalised carriers as float bits.  One clean superframe of two 2k modes, an 8k frame, a second sync_start tag in
    mid-stream, a stream entered at nine places of a superframe, a dropped symbol, TPS words with one and two flipped bits."""
    case, inp, ora, _ = check_case(po, golden, name)
    sf = [t for t in ora["tags"] if t[2] == "superframe_start"]
    assert len(sf) == len(case["sync"]) and sum(e[1] for e in ora["log"]) > 4
    if name.endswith("superframe"):
        assert sum(e[1] for e in ora["log"]) >= 272
    assert all(t[3] == 0xaa for t in sf)


@pytest.mark.parametrize("name", _names("refsig"))
def test_pilot_insertion(po, golden, name):
    """the TX generator's pilot / TPS insertion (oracle/o_tx.c) against reference_signals: the block is fed the payload cells of the generator's symbols, read
    where the block itself puts payload, and must give the generator's symbols back, as float bits, over more than a frame (a superframe in 2k)"""
    check_case(po, golden, name)


@pytest.mark.parametrize("name", _names("chain"))
def test_receive_chain(po, golden, name):
    """the scheduling BETWEEN the blocks that oracle/o_chain.c restates: the reference's receive blocks chained from demod_reference_signals to
    energy_descramble on the FFT items of a loopback, each in its smallest calls, tags handed on by hand, against all eight taps of o_rx_run -- on clean
    streams and on one whose CP lock is lost in mid-superframe (two lock periods: the partial Viterbi block and the partial pair of de-interleaver items in
    front of the new superframe_start tag are dropped, the descrambler goes on).  o_rx_run's Viterbi tap leaves out the bytes the de-interleaver drops."""
    case, inp, ora, _ = check_case(po, golden, name)
    assert all(len(o) > 0 for o in ora["out"]) and len(ora["out"][-1]) >= 100 * 188
    assert inp["rx"]["truncated"] == (1 if "gap" in case else 0)
