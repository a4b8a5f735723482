"""The repair passes behind the chunk decoders (k_viterbi3.hpp: viterbi_check_kernel / viterbi_count_kernel, v3_repair_rows, v3_seq_walk, viterbi_fix_kernel) where chunks really hand
over: a repaired chunk whose decoder arrives at the next chunk in a state other than the one that chunk was checked against, so that fix[] is written, the chunk flagged and the
sequential walk has work -- it runs on into the next chunk, it runs through chunks that were flagged themselves, it rewrites the state a call leaves for the next one.

No stream the chain can decode reaches that at the product's sizes.  Chunks of ONE block of windows (24 bytes) behind the shortest warm-up (48 windows) on garbage -- uniform random
decoder symbols -- do, a dozen times in 12,000 chunks: the single block takes both sizes through its test hooks (dvbt_viterbi_decoder_set_chunk_bytes, _set_warm_windows, _set_verify,
_last_ctl).  The reference is the oracle's one streaming decoder over the same input (o_viterbi_decode); no case allows a differing byte.  The counters of the passes are compared
with the replay of the same passes on the CPU (tests/vitrepairref.py, certified by tests/test_viterbi_handover_model.py): the kernels compare decoder states at the top of window
b0 + 2 of a chunk that starts with byte b0, right behind a renormalisation, the replay the reference's metrics right behind get_output call b0 + 1, minimum subtracted -- the same
trellis position (a block's step 0 is real step 8 w - 10 = the step behind call w - 1) and a canonical vector on either side, so the counts are EQUAL, launch by launch, and asserted so."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vitrepairref as V  # noqa: E402
from test_gpu_viterbi_staging import CONFIGS, IDS  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNKS, MISMATCH, CONFLICT, UNPROVEN, SEQ = 0, 1, 2, 3, 4                   # k_viterbi3.hpp, V3_CTL_*


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    return gr_dvbt_amd


def _oracle(po, c, vin):
    ref = np.zeros(len(vin) * c.m * c.k // (8 * c.n) + 64, np.uint8)
    po.lib().o_viterbi_decode.restype = C.c_size_t
    n = po.lib().o_viterbi_decode(C.byref(c), V.BSIZE, vin.ctypes.data_as(C.c_void_p), C.c_size_t(len(vin)), ref.ctypes.data_as(C.c_void_p))
    return ref[:n]


def _run(g, const, cr, c, vin, calls, mode=1, walk=False, ctl=True, chunk=V.CHUNK, warm=V.WARM):
    """the stream through one block in calls of calls[i] reference blocks: (bytes, the summed counters, the control words behind every call that launched)"""
    d_nsym, d_nout = V.block_sizes(c)
    b = g.Block("viterbi_decoder", const, 0, cr, V.BSIZE, 0, -1)
    b.set_viterbi_chunk_bytes(chunk); b.set_viterbi_warm_windows(warm); b.set_viterbi_verify(mode)
    if walk:
        b.set_viterbi_walk(True)
    outs, ctls, pos = [], [], 0
    for k, nb in enumerate(calls):
        o = np.zeros(nb * d_nout, np.uint8)
        r, cons, _ = b.work(nb * d_nout, nb * d_nsym, vin[pos * d_nsym:(pos + nb) * d_nsym], o, tags=[(0, g.TAG_SUPERFRAME_START, 0xaa)] if k == 0 else [])
        assert cons == nb * d_nsym
        outs.append(o[:r]); pos += nb
        ctls.append(b.viterbi_last_ctl() if (ctl and r > 0) else None)
    proof = b.viterbi_proof()
    b.close()
    return np.concatenate(outs), proof, ctls


def _model(R, l):
    """the replay's (chunks, listed, conflicts, sequential) of one launch l = (grid entry, first chunk, end chunk)"""
    r = R.launch(l[1], l[2])
    return (l[2] - l[1], len(r["listed"]), len(r["flagged"]), r["walked"])


def _gpu(ctl):
    return (ctl[CHUNKS], ctl[MISMATCH], ctl[CONFLICT], ctl[SEQ])


_one = {}


def _one_call(po, g, name):
    """the named input as ONE call with the final check (mode 1), once per process"""
    if name not in _one:
        const, cr, seed, kind = V.INPUTS[name]
        c, nblocks, vin, R, r = V.replay(po, name)
        _one[name] = _run(g, const, cr, c, vin, [nblocks])
    return _one[name]


@pytest.mark.parametrize("name", list(V.INPUTS))
def test_one_call_takes_the_three_launch_path(po, g, name):
    """12,000 chunks in one launch: check, parallel repair (64 workgroups), sequential walk and the final check as launches of their own"""
    const, cr, seed, kind = V.INPUTS[name]
    c, nblocks, vin, R, r = V.replay(po, name)
    out, proof, ctls = _one_call(po, g, name)
    ref = _oracle(po, c, vin)
    model = (R.nch, len(r["listed"]), len(r["flagged"]), r["walked"])
    print(f"{name}, one call: (chunks, listed, conflicts, sequential) GPU {_gpu(ctls[0])} model {model}; differing bytes {int((out != ref).sum()) if len(out) == len(ref) else -1} of {len(ref)}")
    assert len(out) == len(ref) == R.total_out and (out == ref).all(), np.flatnonzero(out != ref)[:5]
    assert proof["not_proven"] == 0 and ctls[0][UNPROVEN] == 0
    assert proof["chunks"] == ctls[0][CHUNKS] == R.nch > V.FIX_SMALL
    assert _gpu(ctls[0]) == model                                          # (the module's docstring: the same position, canonical vectors)
    assert ctls[0][CONFLICT] >= 1 and ctls[0][SEQ] >= 1 and proof["decoded_again"] == ctls[0][MISMATCH] and proof["sequential"] == ctls[0][SEQ]
    if kind is not None:
        assert ctls[0][SEQ] != ctls[0][CONFLICT]                            # isolated flags leave the two equal: a walk ran past its first chunk
    if kind == "continuation":
        assert ctls[0][SEQ] > ctls[0][CONFLICT]
    if kind == "absorption":
        assert ctls[0][SEQ] < ctls[0][CONFLICT]


@pytest.mark.parametrize("name", list(V.INPUTS))
def test_calls_of_at_most_1024_chunks_take_the_fused_path(po, g, name):
    """the same streams in calls of 1021 to 1024 chunks (vitrepairref.fused_blocks: a call of exactly 1024 chunks' worth of bytes can span 1025 chunks of the grid, because the
    carried state stands up to 23 bytes in front of the call): viterbi_fix_kernel, one workgroup, 16 repair rows -- and in one call (of the five inputs' 60) more than 20 listed
    chunks, a second round of the rows"""
    const, cr, seed, kind = V.INPUTS[name]
    c, nblocks, vin, R, r = V.replay(po, name)
    calls = V.cut(nblocks, [V.fused_blocks(c)])
    ls = V.launches(po, name, calls)
    out, proof, ctls = _run(g, const, cr, c, vin, calls)
    ref = _oracle(po, c, vin)
    assert len(out) == len(ref) and (out == ref).all(), np.flatnonzero(out != ref)[:5]
    gpu = [_gpu(x) for x in ctls]
    model = [_model(R, l) for l in ls]
    print(f"{name}, {len(calls)} calls of {calls[0]} blocks: (chunks, listed, conflicts, sequential) per call GPU {gpu} model {model}")
    assert all(x[UNPROVEN] == 0 for x in ctls) and all(V.FIX_SMALL - 3 <= x[CHUNKS] <= V.FIX_SMALL for x in ctls[:-1]) and ctls[-1][CHUNKS] <= V.FIX_SMALL
    if V.CHUNK % V.block_sizes(c)[1] == 0:                                  # (blocks of 6 or 12 bytes; 7/8's 42 make 1021 or 1022 chunks)
        assert any(x[CHUNKS] == V.FIX_SMALL for x in ctls)                  # the largest launch the fused kernel takes
    assert gpu == model
    assert sum(x[CONFLICT] for x in ctls) >= 1 and sum(x[SEQ] for x in ctls) >= 1
    assert proof["decoded_again"] == sum(x[MISMATCH] for x in ctls) and proof["sequential"] == sum(x[SEQ] for x in ctls) and proof["chunks"] == sum(x[CHUNKS] for x in ctls)
    big, k = V.fused_call_above_20(po)
    assert big in V.INPUTS                                                  # (tests/test_viterbi_handover_model.py holds that one exists)
    if name == big:
        assert ctls[k][MISMATCH] > 20 > 16 and ctls[k][CHUNKS] <= V.FIX_SMALL, ctls[k]


def _single_call_chunks(c, cr, nb):
    return -(-(nb * V.block_sizes(c)[1] - V.NTB[cr]) // V.CHUNK)


def test_the_boundary_between_the_fused_and_the_three_launch_path(po, g):
    """the head of one stream as one call of the most blocks that make at most 1024 chunks (fused) and as one call of the fewest that make more (three launches): the same bytes over
    the common prefix, and the counters the replay gives for either launch -- conflicts and a walk in both"""
    for name in V.INPUTS:                                                   # the first input with a hand-over among its first thousand chunks
        const, cr, seed, kind = V.INPUTS[name]
        c, nblocks, vin, R, r = V.replay(po, name)
        d_nsym, d_nout = V.block_sizes(c)
        nb_lo = max(nb for nb in range(1, 6000) if _single_call_chunks(c, cr, nb) <= V.FIX_SMALL)
        nb_hi = nb_lo + 1
        n_lo, n_hi = _single_call_chunks(c, cr, nb_lo), _single_call_chunks(c, cr, nb_hi)
        m_lo, m_hi = _model(R, (None, 0, n_lo)), _model(R, (None, 0, n_hi))
        if m_lo[2] >= 1 and m_lo[3] >= 1:
            break
    assert n_lo <= V.FIX_SMALL < n_hi <= V.FIX_SMALL + 2 and m_lo[2] >= 1 and m_lo[3] >= 1
    res = {}
    for nb in (nb_lo, nb_hi):
        x = np.ascontiguousarray(vin[:nb * d_nsym])
        out, proof, ctls = _run(g, const, cr, c, x, [nb])
        ref = _oracle(po, c, x)
        assert len(out) == len(ref) and (out == ref).all(), (nb, np.flatnonzero(out != ref)[:5])
        assert proof["not_proven"] == 0
        res[nb] = (out, _gpu(ctls[0]))
    print(f"{name}: one call of {nb_lo} blocks, (chunks, listed, conflicts, sequential) GPU {res[nb_lo][1]} model {m_lo}; of {nb_hi} blocks GPU {res[nb_hi][1]} model {m_hi}")
    assert (res[nb_lo][0] == res[nb_hi][0][:len(res[nb_lo][0])]).all()
    assert res[nb_lo][1] == m_lo and res[nb_hi][1] == m_hi
    assert all(res[nb][1][2] >= 1 and res[nb][1][3] >= 1 for nb in res)
    if m_lo[1:] == m_hi[1:]:
        assert res[nb_lo][1][1:] == res[nb_hi][1][1:]


@pytest.mark.parametrize("name", ["qam64-2/3-continuation", "qam64-7/8"])
def test_the_state_is_carried_across_calls_that_end_in_repaired_chunks(po, g, name):
    """calls of 1, 2, 3 and 5 reference blocks (2/3: 12 to 60 bytes, launches of one to four chunks): every call's chunk 0 starts from the state the call before left, and that state
    is rewritten by the repair of a call's last chunk (v3_repair_rows / v3_seq_walk, carry_out) -- in the calls that end in a listed chunk, which the replay names.  The state is
    left at the last top of a block of windows in front of the call's end: with chunks of 24 bytes at the last chunk's first window (carry_rel 0) or -- where the call ends on the
    grid, which a whole number of blocks minus ntraceback bytes does at rate 7/8 only (42 n - 24) -- behind its last (carry_rel 24)"""
    const, cr, seed, kind = V.INPUTS[name]
    c, nblocks, vin, R, r = V.replay(po, name)
    calls = V.cut(nblocks, [1, 2, 3, 5])
    ls = [l for l in V.launches(po, name, calls) if l is not None]
    listed = [R.check(l[1], l[2]) for l in ls]
    ends_listed = sum(1 for l, x in zip(ls, listed) if l[2] - 1 in x)
    rels = {(l[0][2] - (l[0][0] + (l[0][3] - 1) * V.CHUNK)) // 24 * 24 for l in ls}
    print(f"{name} in {len(calls)} calls of 1, 2, 3, 5 blocks: {sum(len(x) for x in listed)} chunks listed, {ends_listed} calls end in a listed chunk; carry_rel takes {sorted(rels)}")
    assert ends_listed >= 5 and rels == ({0, 24} if name == "qam64-7/8" else {0})
    out, proof, _ = _run(g, const, cr, c, vin, calls, ctl=False)
    ref = _oracle(po, c, vin)
    assert len(out) == len(ref) and (out == ref).all(), np.flatnonzero(out != ref)[:5]
    assert proof["decoded_again"] == sum(len(x) for x in listed) and proof["chunks"] == sum(l[2] - l[1] for l in ls)
    one = _one_call(po, g, name)[0]
    assert len(one) == len(out) and (one == out).all()


def test_every_mode_of_the_passes(po, g):
    """dvbt_viterbi_decoder_set_verify on one stream: the modes that repair give the streaming decoder's bytes; the proof alone (2) leaves what the plain chunk decoders wrote and
    counts what it could not prove; the plain decoders (-1, chunk 0 of the launch at the call's first byte) differ in a few hundred bytes"""
    name = "qam64-2/3-continuation"
    const, cr, seed, kind = V.INPUTS[name]
    c, nblocks, vin, R, r = V.replay(po, name)
    ref = _oracle(po, c, vin)
    res = {1: _one_call(po, g, name)}
    for mode in (-1, 0, 2, 3, 4):
        res[mode] = _run(g, const, cr, c, vin, [nblocks], mode=mode)
    diff = {m: int((res[m][0] != ref).sum()) if len(res[m][0]) == len(ref) else -1 for m in res}
    print(f"{name}: bytes that differ from the streaming decoder by mode {diff} (the replay's plain chunk decoders: {R.plain_wrong}); counters",
          {m: (res[m][1], _gpu(res[m][2][0]), res[m][2][0][UNPROVEN]) for m in res})
    for m in (0, 1, 3, 4):
        assert diff[m] == 0, diff
    assert res[0][1]["not_proven"] == -1 and all(res[m][1]["not_proven"] == 0 for m in (1, 3, 4))
    assert res[2][1]["not_proven"] == len(r["listed"]) > 0 and diff[2] == R.plain_wrong > 0
    assert (res[2][0] == R.plain[:len(ref)]).all()                          # byte for byte what the replay's plain chunk decoders write
    assert 0 < diff[-1] < len(ref) // 100
    assert res[3][1]["sequential"] >= res[3][1]["decoded_again"] == len(r["listed"])
    assert res[0][1]["decoded_again"] == res[4][1]["decoded_again"] == len(r["listed"]) and res[0][1]["sequential"] == r["walked"]
    assert res[4][2][0][CONFLICT] >= len(r["listed"]) - 1 and res[4][1]["sequential"] >= 1


@pytest.mark.parametrize("const,cr", CONFIGS, ids=IDS)
def test_every_traceback_depth(po, g, const, cr):
    """1,000 chunks of garbage for every constellation and rate (ntraceback 5, 9, 10, 15, 24; every puncture period): the bytes, and nothing left unproven"""
    c, nblocks, vin = V.stream(po, const, cr, 100 + 5 * const + cr, decoded=24000)
    out, proof, ctls = _run(g, const, cr, c, vin, [nblocks])
    ref = _oracle(po, c, vin)
    print(f"c{const}-r{cr}: (chunks, listed, conflicts, sequential) {_gpu(ctls[0])}")
    assert len(out) == len(ref) > 23000 and (out == ref).all(), np.flatnonzero(out != ref)[:5]
    assert proof["not_proven"] == 0 and proof["chunks"] == -(-len(ref) // V.CHUNK)


def test_the_passes_with_the_traceback_shortcut_switched_off(po, g):
    """dvbt_viterbi_decoder_set_walk(1): every chain walks its hops, in the chunk decoders and in the repairs; the same bytes, the same counters"""
    name = next(iter(V.INPUTS))
    const, cr, seed, kind = V.INPUTS[name]
    c, nblocks, vin, R, r = V.replay(po, name)
    out, proof, ctls = _run(g, const, cr, c, vin, [nblocks], walk=True)
    one = _one_call(po, g, name)
    assert len(out) == len(one[0]) and (out == one[0]).all() and (out == _oracle(po, c, vin)).all()
    assert proof == one[1] and ctls[0][:5] == one[2][0][:5]
