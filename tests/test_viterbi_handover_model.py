"""(no GPU) What the reference alone certifies about the inputs of tests/test_gpu_viterbi_handover.py: garbage decoder symbols through chunks of 24 bytes behind a warm-up of 48 windows,
replayed by tests/vitrepairref.py on the kernels' own grid (chunk c = bytes [24 c, 24 c + 24), its decoder started with equal metrics at the top of window 24 c + 2 - 48).  On these
inputs repaired chunks do NOT arrive in the state their successor was checked against: chunks are handed to the walk, the walk runs on into the next chunk (continuation: it decodes
more chunks than were flagged) or through a chunk that was flagged itself (absorption: fewer) -- and the assembled bytes are the streaming decoder's, every one.

The conditions below are the selection rule of the seeds in vitrepairref.INPUTS: for each case the seeds 1, 2, 3, ... were tried in turn and the first that meets them was taken
(QAM64 2/3: seed 1 continues, seed 5 is the first of at least 10 flagged chunks whose walk decodes fewer than were flagged; QPSK 2/3 and QAM16 1/2: seed 1)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vitrepairref as V  # noqa: E402


@pytest.mark.parametrize("name", list(V.INPUTS))
def test_inputs_reach_the_hand_over_and_the_replay_is_the_streaming_decoder(po, name):
    const, cr, seed, kind = V.INPUTS[name]
    c, nblocks, vin, R, r = V.replay(po, name)
    d_nsym, d_nout = V.block_sizes(c)
    listed, flagged, walked = len(r["listed"]), len(r["flagged"]), r["walked"]
    print(f"{name} (seed {seed}): {R.nch} chunks, {listed} listed ({R.plain_wrong} bytes of the plain chunk decoders differ), {flagged} handed to the walk, {r['starts']} walks, {walked} decoded by them")
    assert R.total_out == nblocks * d_nout - V.NTB[cr] and R.nch == -(-R.total_out // V.CHUNK) >= 12000
    n = R.total_out
    assert (r["out"][:n] == R.full[:n]).all(), int((r["out"][:n] != R.full[:n]).sum())
    for i in range(1, R.nch):                                               # the chain of states is consistent and IS the streaming decoder's
        assert (r["own"][i] == r["pred"][i]).all() and (r["pred"][i] == R.truth[i]).all(), i
    assert flagged >= (3 if (const, cr) == (1, 0) else 10)
    assert walked >= r["starts"] >= 1
    if kind == "continuation":
        assert walked > flagged
    if kind == "absorption":
        assert walked < flagged
    assert R.plain_wrong > 100


def test_a_fused_launch_lists_more_than_twenty(po):
    """calls of at most 1024 chunks (viterbi_fix_kernel): one of them, over the five inputs, lists more than 20 chunks -- more than the fused repair's 16 rows take in one round"""
    name, k = V.fused_call_above_20(po)
    print("the first call of at most 1024 chunks that lists more than 20:", name, "call", k)
    assert name in V.INPUTS


def test_the_call_grid_is_the_chunk_grid_at_24_bytes():
    """with chunks of one block of windows the carried state stands at a multiple of 24 in every call, at most 23 bytes in front of the call's first byte"""
    for nt, d_nout in ((9, 12), (5, 6), (24, 42)):
        calls = V.call_grid(nt, d_nout, [1, 2, 3, 5] * 50)
        assert calls[0] is None or calls[0][0] == 0
        for g in calls:
            if g is not None:
                g0, lo, hi, chunks = g
                assert g0 % 24 == 0 and 0 <= lo - g0 < 24 and hi > lo and chunks == -(-(hi - g0) // 24)
