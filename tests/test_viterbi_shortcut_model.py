"""The traceback's shortcut over chained best states (gr_dvbt_amd/csrc/k_viterbi3.hpp, header comment), as a plain numpy model -- no GPU.

A K = 7 decoder in the reference's layout (d_viterbi.c:503-521, 699-724): 64 metrics, one path byte per state and window of 8 steps (the survivor's last eight decisions:
byte >> 2 = its state at the window's start), the best state of a window = the first index of the maximum metric, and the byte of call w = the path byte reached from
best(w) by ntraceback - 1 hops, byte >> 2 each.  The rule: link(u) holds when one hop from best(u) lands on best(u - 1); where link(u) holds for every u in
[w - (ntraceback - 2), w] the walk of call w ends at best(w - ntraceback + 1), and the call's byte is that window's path byte at its own best state.  For all five rates at
bit-error rates 0, 0.5 %, 2 % and 6 % the two bytes are compared wherever the links hold, and the neighbouring choices of the output window (one further, one nearer) are shown
to be wrong -- which pins the range and the window.  The share of calls on the shortcut is printed per rate and error rate, per call and per block of 24 windows the way the
kernel decides (every link of the block and of the block before it)."""
import numpy as np
import pytest

K_OF_RATE, NTB = (1, 2, 3, 5, 7), (5, 9, 10, 15, 24)
PUNCT = ((1, 1), (1, 1, 0, 1), (1, 1, 0, 1, 1, 0), (1, 1, 0, 1, 1, 0, 0, 1, 1, 0), (1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0))
BERS = (0.0, 0.005, 0.02, 0.06)
NBYTES = 600                                                         # 25 blocks of 24 windows
PAR = np.array([bin(i).count("1") & 1 for i in range(128)], np.int64)
SR = np.arange(64)                                                   # new state ns reached from ns >> 1 (register ns) or (ns >> 1) + 32 (register ns + 64)
X0, Y0, X1, Y1 = PAR[SR & 0x4f], PAR[SR & 0x6d], PAR[(SR + 64) & 0x4f], PAR[(SR + 64) & 0x6d]
P0, P1 = SR >> 1, (SR >> 1) + 32


def _received(cr, ber, seed):
    """(data bytes, per step: the two received bits and their keep flags)"""
    rng = np.random.RandomState(seed)
    data = rng.randint(0, 256, NBYTES).astype(np.uint8)
    bits = np.unpackbits(data)
    sr, coded = 0, np.empty((len(bits), 2), np.int64)
    for t, b in enumerate(bits):
        sr = ((sr << 1) | int(b)) & 127
        coded[t] = PAR[sr & 0x4f], PAR[sr & 0x6d]
    keep = np.resize(np.array(PUNCT[cr], np.int64), 2 * len(bits)).reshape(-1, 2)
    flips = (rng.rand(len(bits), 2) < ber).astype(np.int64)
    return data, coded ^ flips, keep


def _decode(rx, keep):
    """path bytes tab[w][state] and best[w] for every window"""
    nwin = len(rx) // 8
    M, path = np.zeros(64, np.int64), np.zeros(64, np.int64)
    tab, best = np.zeros((nwin, 64), np.int64), np.zeros(nwin, np.int64)
    for t in range(nwin * 8):
        (r0, r1), (k0, k1) = rx[t], keep[t]
        ma = M[P0] + k0 * (X0 == r0) + k1 * (Y0 == r1)
        mb = M[P1] + k0 * (X1 == r0) + k1 * (Y1 == r1)
        lower = ma > mb                                              # a tie goes to the upper predecessor (d_viterbi.c:508-521)
        M = np.where(lower, ma, mb)
        path = ((np.where(lower, path[P0], path[P1]) << 1) | np.where(lower, 0, 1)) & 255     # the decision = the bit that leaves the register (:515-521)
        if t % 8 == 7:
            w = t // 8
            tab[w], best[w] = path, int(np.argmax(M))                # argmax: the first index of the maximum (:699-711)
            M = M - M.min()
    return tab, best


def _walk(tab, best, w, ntb):
    s = best[w]
    for i in range(ntb - 1):
        s = tab[w - i][s] >> 2
    return tab[w - ntb + 1][s]


@pytest.mark.parametrize("cr", range(5), ids=["1/2", "2/3", "3/4", "5/6", "7/8"])
def test_shortcut_byte_is_the_walked_byte(cr):
    ntb = NTB[cr]
    for ber in BERS:
        data, rx, keep = _received(cr, ber, 40 + cr)
        tab, best = _decode(rx, keep)
        nwin = len(best)
        link = np.zeros(nwin, bool)
        link[1:] = (tab[np.arange(1, nwin), best[1:]] >> 2) == best[:-1]
        calls = short = other_further = other_nearer = 0
        for w in range(ntb - 1, nwin):
            walked = _walk(tab, best, w, ntb)
            calls += 1
            if link[w - (ntb - 2):w + 1].all():                      # the hops from w, w - 1, .., w - (ntb - 2)
                short += 1
                assert tab[w - ntb + 1][best[w - ntb + 1]] == walked, (ber, w)
                other_nearer += tab[w - ntb + 2][best[w - ntb + 2]] != walked
                if w - ntb >= 0:
                    other_further += tab[w - ntb][best[w - ntb]] != walked
        if ber == 0.0:
            got = np.array([_walk(tab, best, w, ntb) for w in range(ntb - 1, nwin)])
            sent = np.unpackbits(data)
            # the path byte of window u holds the inputs of steps 8u - 6 .. 8u + 1
            want = np.array([np.packbits(sent[8 * u - 6:8 * u + 2])[0] for u in range(1, nwin - ntb + 1)])
            assert (got[1:] == want).all()
            assert short >= calls - 2 * ntb, (short, calls)           # a clean stream chains up everywhere behind the cold start
        # one window further or nearer is another byte (random data: all but 1 in 256 differ)
        assert short == 0 or (other_nearer > short // 2 and other_further > short // 2), (ber, short, other_nearer, other_further)
        # the kernel's decision: a block of 24 windows is on the shortcut when all its links and all links of the block before hold
        blk_ok = [link[b:b + 24].all() for b in range(0, nwin - 23, 24)]
        blk_fast = sum(blk_ok[i] and blk_ok[i - 1] for i in range(1, len(blk_ok)))
        print(f"rate {ids(cr)} ber {ber:5.3f}: {short}/{calls} calls on the shortcut ({100.0 * short / calls:.1f} %), links that hold {100.0 * link[1:].mean():.1f} %, "
              f"blocks of 24 on the shortcut as the kernel decides {blk_fast}/{len(blk_ok) - 1}")


def ids(cr):
    return ("1/2", "2/3", "3/4", "5/6", "7/8")[cr]
