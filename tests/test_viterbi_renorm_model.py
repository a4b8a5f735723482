"""The range of the Viterbi decoder's 8-bit metric field between two renormalisations (gr_dvbt_amd/csrc/k_viterbi3.hpp, the range note in the header), as an exact-integer
model -- numpy, no GPU.

The kernel keeps a cell as (2M + bias) << 8 | path byte and adds / subtracts the branch deltas with packed 16-bit arithmetic that wraps: the field (bits 15:8) of every cell, and
of both candidates X = cell + delta, Y = cell - delta of every step, must stay inside int8.  The last window of every group of V3_RENORM_EVERY sets the best field back to
V3_RENORM_BEST (v3_window_end); a decoder starts with every field there.  Both constants are read from the header.

The model keeps, per state s, E[s] = 2M[s] + the common offset (even) and forms the field as the kernel holds it in front of step t: E[s] + bit 8, where bit 8 is the tie-break
bit that is armed there at that step -- three steps at a time (v3_step's ST): in front of the steps 0..2 of a window the bias of its step 2, in front of 3..5 that of step 5, then
those of steps 6 and 7.  The cell of state s at phase p is rotr6(s, p) and its bias for phase Q is cell bit 5 - Q, so bit 8 = state bit (5 - Q + p) mod 6.  At the compare of
a step the bit that decides is the predecessor's own bias (1 = upper state, i + 32): candidates 2M_lower + d and 2M_upper + 1 - d, the larger one wins.

Beside it runs a second decoder that never renormalises, on Python integers (object arrays: unbounded), with the reference's tie rule written out (a tie goes to the upper
predecessor, d_viterbi.c:508-521; the best state is the first index of the maximum, :699-711).  All five rates x six streams run side by side as rows of one array."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "gr_dvbt_amd", "csrc", "k_viterbi3.hpp")).read()
EVERY = int(re.search(r"constexpr int V3_RENORM_EVERY = (-?\d+);", HEADER).group(1))
BEST = int(re.search(r"constexpr int V3_RENORM_BEST = (-?\d+);", HEADER).group(1))
BLK = int(re.search(r"constexpr int V3_BLK = (\d+);", HEADER).group(1))

PUNCT = ((1, 1), (1, 1, 0, 1), (1, 1, 0, 1, 1, 0), (1, 1, 0, 1, 1, 0, 0, 1, 1, 0), (1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0))
RATES = ("1/2", "2/3", "3/4", "5/6", "7/8")
STREAMS = ("clean", "2 % flipped", "6 % flipped", "20 % flipped", "random", "48 windows random / 48 clean")
STRETCH = 48 * 8                                                     # steps of a stretch of the alternating stream
NSTEPS = 14 * STRETCH                                                # 5,376 steps = 672 windows = 112 groups of six
PAR = np.array([bin(i).count("1") & 1 for i in range(128)], np.int64)
NS = np.arange(64)                                                   # new state ns is reached from ns >> 1 (register ns) or (ns >> 1) + 32 (register ns + 64)
LX, LY = PAR[NS & 0x4f], PAR[NS & 0x6d]                              # the label of the branch from the lower predecessor; the upper one's is its complement
P_LO, P_HI = NS >> 1, (NS >> 1) + 32
OWN = (2 * NS) & 63                                                  # a state's own branch (to 2s): |delta| is the same on its other branch


def _streams():
    """rx[run, step, 2], keep[run, step, 2] for the 30 runs (rate-major)"""
    rx = np.zeros((len(RATES) * len(STREAMS), NSTEPS, 2), np.int64)
    keep = np.zeros_like(rx)
    for cr in range(len(RATES)):
        for k, ber in enumerate((0.0, 0.02, 0.06, 0.20, None, None)):
            rng = np.random.RandomState(900 + 10 * cr + k)
            bits = rng.randint(0, 2, NSTEPS)
            sr, coded = 0, np.empty((NSTEPS, 2), np.int64)
            for t in range(NSTEPS):
                sr = ((sr << 1) | int(bits[t])) & 127
                coded[t] = PAR[sr & 0x4f], PAR[sr & 0x6d]
            noise = rng.randint(0, 2, (NSTEPS, 2))
            if ber is not None:
                r = coded ^ (rng.rand(NSTEPS, 2) < ber)
            elif k == 4:
                r = noise
            else:
                r = np.where(((np.arange(NSTEPS) // STRETCH) % 2 == 0)[:, None], noise, coded)
            rx[cr * len(STREAMS) + k] = r
            keep[cr * len(STREAMS) + k] = np.resize(np.array(PUNCT[cr], np.int64), 2 * NSTEPS).reshape(-1, 2)
    return rx, keep


def _q_of_step(t):
    """the phase whose tie-break bit stands at bit 8 in front of step t (v3_step: ST = 3 after a window's 3rd step, 1 after the 6th, 4 after the 7th, 2 after the last)"""
    u = t % 8
    return (t - u + 2) % 6 if u < 3 else (t - u + 5) % 6 if u < 6 else t % 6


@pytest.fixture(scope="module")
def runs():
    """one pass over all runs: per run the extremes of the field and of the candidates, the best field's steps, the largest spread, and whether every decision and every window's
    best state was the unbounded decoder's"""
    rx, keep = _streams()
    R = rx.shape[0]
    E = np.full((R, 64), BEST, np.int64)                             # the kernel's start state: every field at V3_RENORM_BEST
    M2 = np.empty((R, 64), object)
    M2[:] = 0
    rows = np.arange(R)[:, None]
    f_lo = np.full(R, 1 << 30)
    f_hi = -f_lo
    c_lo, c_hi = f_lo.copy(), f_hi.copy()
    rise_lo, rise_hi, spread = f_lo.copy(), f_hi.copy(), np.zeros(R, np.int64)
    same_dec, same_best = np.ones(R, bool), np.ones(R, bool)
    for t in range(NSTEPS):
        p, q = t % 6, _q_of_step(t)
        # delta of the branch from the lower predecessor into ns: 2 x (agreements - disagreements) over the kept symbols; from the upper one it is the negative
        d = 2 * (keep[:, t, 0:1] * (1 - 2 * (LX[None, :] ^ rx[:, t, 0:1])) + keep[:, t, 1:2] * (1 - 2 * (LY[None, :] ^ rx[:, t, 1:2])))
        field = E + ((NS >> ((5 - q + p) % 6)) & 1)[None, :]
        dabs = np.abs(d[:, OWN])
        f_lo, f_hi = np.minimum(f_lo, field.min(1)), np.maximum(f_hi, field.max(1))
        c_lo, c_hi = np.minimum(c_lo, (field - dabs).min(1)), np.maximum(c_hi, (field + dabs).max(1))
        spread = np.maximum(spread, field.max(1) - field.min(1))
        # the kernel's compare: bit 8 of both candidates is the predecessor's own bias at this step
        ca, cb = E[:, P_LO] + d, E[:, P_HI] + 1 - d
        lower = ca > cb
        top = E.max(1)
        E = np.where(lower, ca, cb - 1)
        rise = E.max(1) - top
        rise_lo, rise_hi = np.minimum(rise_lo, rise), np.maximum(rise_hi, rise)
        # the second decoder: Python integers, no offset ever removed, the tie rule written out
        dobj = d.astype(object)
        ma, mb = M2[:, P_LO] + dobj, M2[:, P_HI] - dobj
        lower2 = (ma > mb).astype(bool)
        M2 = np.where(lower2, ma, mb)
        same_dec &= (lower == lower2).all(1)
        if t % 8 == 7:
            w = t // 8
            key = (E + 1 - (NS >> 5)[None, :]) * 256 + 63 - NS[None, :]           # v3_window_end: among equal 2M the lower states first, then the smaller state
            best2 = (M2 == M2.max(1)[:, None]).argmax(1)                           # the first index of the maximum
            same_best &= key.argmax(1) == best2
            if w % EVERY == EVERY - 1:
                E = E - (E.max(1) - BEST)[:, None]
    assert all(type(x) is int for x in M2.reshape(-1)[:64])
    return dict(f_lo=f_lo, f_hi=f_hi, c_lo=c_lo, c_hi=c_hi, rise_lo=rise_lo, rise_hi=rise_hi, spread=spread, same_dec=same_dec, same_best=same_best)


def test_constants_satisfy_the_inequalities():
    assert BLK % EVERY == 0
    assert BEST % 2 == 0                                             # bit 8 is the tie-break bit
    assert BEST - 49 - 4 >= -128
    assert BEST + 1 + 4 * 8 * EVERY + 4 <= 127
    assert NSTEPS >= 5000 and NSTEPS % (8 * EVERY) == 0


@pytest.mark.parametrize("stream", range(len(STREAMS)), ids=[s.replace(" ", "_").replace("/", "-") for s in STREAMS])
@pytest.mark.parametrize("cr", range(len(RATES)), ids=RATES)
def test_field_stays_inside_int8(runs, cr, stream):
    i = cr * len(STREAMS) + stream
    r = {k: v[i] for k, v in runs.items()}
    print(f"rate {RATES[cr]} {STREAMS[stream]}: field [{r['f_lo']}, {r['f_hi']}], candidates [{r['c_lo']}, {r['c_hi']}], spread {r['spread']}, "
          f"best per step +{r['rise_lo']}..+{r['rise_hi']}")
    assert -128 <= r["c_lo"] <= r["f_lo"] and r["f_hi"] <= r["c_hi"] <= 127
    assert r["f_lo"] >= BEST - 49 and r["f_hi"] <= BEST + 1 + 4 * 8 * EVERY and r["c_lo"] >= BEST - 53 and r["c_hi"] <= BEST + 5 + 4 * 8 * EVERY   # the range note's own bounds
    assert 0 <= r["rise_lo"] and r["rise_hi"] <= 4                   # the best never decreases and rises by at most 4 per step
    assert r["spread"] <= 49
    assert r["same_dec"] and r["same_best"]                          # every decision and every window's best state are the unbounded decoder's
