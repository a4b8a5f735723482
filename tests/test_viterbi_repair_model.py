"""The repair passes that make the HIP chunk decoders the reference's ONE streaming decoder (k_viterbi3.hpp: viterbi_check_kernel, viterbi_repair_kernel, viterbi_repair_seq_kernel;
DESIGN.md 2), replayed on the CPU with the oracle's decoder (oracle/o_viterbi.c, pinned to the reference's own kernels by tests/test_oracle_ref_viterbi.py) in the reference's own
state representation -- the 64 path metrics right behind a get_output call (lib/d_viterbi.c:728-732 has just subtracted their minimum and cleared the path bytes):

  own[c]   state of chunk c's decoder (started W windows early from zero metrics) at its chunk's first window
  pred[c]  state there of the decoder whose bytes fill chunk c - 1
  check    the chunks with own[c] != pred[c]
  repair   each of them decoded again from pred[c] (o_viterbi_decode_from), own[c] = pred[c]; where the state it reaches at chunk c + 1 is not pred[c + 1]: fix[c + 1], flagged
  walk     one decoder, in stream order over the flagged chunks: from fix[c] through chunk c, on through c + 1 unless it arrives in own[c + 1]

With chunks of 42 windows and a warm-up of 10 on garbage the decoders rarely merge in time: most chunks are listed, repaired decoders do not arrive where the unproven ones did,
the walk has work -- the hand-overs that real chunk sizes (thousands of windows) never reach.  Whatever the sizes: the assembled bytes are the streaming decoder's, every one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vitrepairref  # noqa: E402

UNIT_IN, UNIT_OUT = vitrepairref.UNITS[(6, 7)]          # QAM64 7/8: 24 trellis bits' worth x 14 = the smallest stretch that is whole in bytes in, bytes out, puncture periods and 16-bit output cadences


@pytest.mark.parametrize("Q,W,kind,seed", [(2, 10, "garbage", 11), (2, 10, "garbage", 12), (2, 10, "garbage", 13), (1, 5, "garbage", 14), (1, 5, "6 %", 15), (2, 24, "6 %", 11),
                                           (8, 24, "garbage", 11), (36, 72, "6 %", 11)],
                         ids=["chunks of 42 windows, warm-up 10, garbage", "the same, seed 12", "the same, seed 13", "21 / 5, garbage", "21 / 5, bit error rate 6 %", "42 / 24, bit error rate 6 %",
                              "168 / 24, garbage", "756 / 72 (the product's warm-up), 6 %"])
def test_check_repair_and_walk_give_the_streaming_decoder(po, Q, W, kind, seed):
    c = po.cfg(po.QAM64, po.C7_8, po.T2k)
    B = UNIT_OUT * Q                                                        # chunk size in bytes = windows
    nunits = 40 * Q if Q <= 8 else 12 * Q
    rng = np.random.RandomState(seed)
    if kind == "garbage":
        vin = rng.randint(0, 64, nunits * UNIT_IN).astype(np.uint8)
    else:
        ibits = c.payload * c.m * c.k // c.n
        iq = po.tx(c, po.make_ts((272 * ibits * 2) // (204 * 8), 5), lead_in=500, tail=3 * c.N)
        vin = po.rx(c, iq, want=("bitdeint",))["bitdeint"].reshape(-1)[:nunits * UNIT_IN].copy()
        for b in range(c.m):
            vin ^= (rng.rand(len(vin)) < 0.06).astype(np.uint8) << b
    vin = np.ascontiguousarray(vin)
    nch = nunits // Q - 2                                                   # chunks c = 0 .. nch - 1; chunk c = bytes [c B + W - 1, (c + 1) B + W - 1)
    # ---- the streaming decoder, the chunk decoders (chunk 0 IS the streaming decoder: it starts the stream; chunk c >= 1 starts W windows early from zero metrics), check, repair, walk
    R = vitrepairref.Replay(po, c, B, W, vin, start="fresh", nch=nch)
    assert R.nfull >= nch * B + W - 1
    r = R.launch()
    out, full, own, pred, truth, listed, walked, plain_wrong = r["out"], R.full, r["own"], r["pred"], R.truth, r["listed"], r["walked"], R.plain_wrong
    flagged = np.zeros(nch + 1, bool); flagged[r["flagged"]] = True
    # ---- every byte is the streaming decoder's; the chain of states is consistent and IS the streaming decoder's
    n = nch * B + W - 1
    print(f"{nch} chunks of {B} windows, warm-up {W}, {kind}: {len(listed)} listed ({plain_wrong} bytes of the plain chunk decoders differ), {int(flagged.sum())} handed to the walk, {walked} decoded by it")
    assert (out[:n] == full[:n]).all(), int((out[:n] != full[:n]).sum())
    for cc in range(1, nch):
        assert (own[cc] == pred[cc]).all() and (pred[cc] == truth[cc]).all(), cc
    if Q <= 2 and kind == "garbage":
        assert len(listed) > nch // 10                                        # the small sizes list many chunks (and, on some seeds, reach the hand-over and the walk: printed)
    if (Q, W, seed) in ((2, 10, 11), (1, 5, 14)):
        assert flagged.sum() > 0 and walked > 0
    if Q == 36:
        assert len(listed) < nch // 2 and walked == 0                         # the product's sizes (a dozen chunks here): few listed if any, none handed on
