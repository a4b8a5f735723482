"""Staging's pair table (gr_dvbt_amd/csrc/k_viterbi3.hpp: v3_step_word, v3_init_lut and the index chain of stage_words), restated in numpy.

A step's word is a function of e = (keep flags of its two symbols) << 2 | the next two received bits (v3_step_word: the 16-entry table every round up to 12 looked up once
per step).  The pair table is keyed by two steps at once, key = (four keep flags) << 4 | the next four received bits, oldest on top; its entry holds the first step's word and
the second step's, taken behind the bits the first step consumed (one per kept symbol).  A lane walks its twelve steps as six links: key from the low four bits of the keep
mask and the top four bits of its 32-bit window, then the window moves up by the number of kept symbols of both steps.
 * all 256 keys: the two words of an entry are the 16-entry table applied twice, the first step's kept symbols consumed in between;
 * all five puncture patterns, every phase of the period, the clamps lo / hi of 0..12 leading / real steps (stage_words' kmask at the stream's ends) and random 32-bit
   windows: six pair look-ups give the twelve words of twelve single look-ups, and the window stands at the same position behind them."""
import numpy as np
import pytest

PUNCT = ((1, 1), (1, 1, 0, 1), (1, 1, 0, 1, 1, 0), (1, 1, 0, 1, 1, 0, 0, 1, 1, 0), (1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0))
SPL = 12                                                             # steps per lane and block


def step_word(e):
    """v3_step_word: the doubled deltas of the four label classes, one byte each"""
    k0, k1, t1, t0 = (e >> 2) & 1, (e >> 3) & 1, (e >> 1) & 1, e & 1
    u0 = 1 - 2 * t1 if k0 else 0
    u1 = (1 - 2 * (t0 if k0 else t1)) if k1 else 0
    d = [2 * (u0 + u1), 2 * (-u0 + u1), 2 * (u0 - u1), 2 * (-u0 - u1)]
    return sum((x & 0xff) << (8 * i) for i, x in enumerate(d))


def pair_entry(e):
    """v3_init_lut: entry e of the pair table"""
    k4, t = e >> 4, e & 15
    used = bin(k4 & 3).count("1")
    return step_word(((k4 & 3) << 2) | (t >> 2)), step_word((k4 & 12) | (((t << used) >> 2) & 3))


def test_an_entry_is_the_single_table_applied_twice():
    single = [step_word(e) for e in range(16)]
    for key in range(256):
        keep, win = key >> 4, (key & 15) << 28                       # the four bits on top of a 32-bit window
        words = []
        for s in range(2):
            k2 = (keep >> (2 * s)) & 3
            words.append(single[(k2 << 2) | (win >> 30)])
            win = (win << bin(k2).count("1")) & 0xffffffff
        assert tuple(words) == pair_entry(key), key


def test_the_single_table_is_what_a_step_needs():
    """the sixteen words against the definition: class c of a step has the labels (c & 1, c >> 1); its delta is the sum over the kept symbols of +1 for an agreeing received
    bit and -1 for a disagreeing one, doubled; a punctured symbol counts nothing; the first kept symbol takes the first of the next received bits"""
    for e in range(16):
        keep, bits = [(e >> 2) & 1, (e >> 3) & 1], [(e >> 1) & 1, e & 1]
        rx, nxt = [None, None], 0
        for s in range(2):
            if keep[s]:
                rx[s] = bits[nxt]
                nxt += 1
        for c in range(4):
            lab = (c & 1, c >> 1)
            d = sum((1 if rx[s] == lab[s] else -1) for s in range(2) if keep[s])
            assert (step_word(e) >> (8 * c)) & 0xff == (2 * d) & 0xff, (e, c)


@pytest.mark.parametrize("cr", range(5))
def test_six_pair_lookups_are_twelve_single_ones(cr):
    p = PUNCT[cr]
    plen = len(p)
    rep = sum(p[i % plen] << i for i in range(64))                   # VitParams.punct_rep
    single = [step_word(e) for e in range(16)]
    pairs = [pair_entry(e) for e in range(256)]
    rng = np.random.RandomState(1300 + cr)
    n = 0
    for ph in range(plen):
        for lo in range(SPL + 1):
            for hi in range(lo, SPL + 1):
                kmask = (((rep >> ph) << (2 * lo)) & ((1 << (2 * hi)) - 1) & ~((1 << (2 * lo)) - 1)) & 0xffffffff
                for win0 in [0, 0xffffffff] + [int(x) for x in rng.randint(0, 2 ** 32, 6, dtype=np.uint64)]:
                    win, a = win0, []
                    for i in range(SPL):
                        k2 = (kmask >> (2 * i)) & 3
                        a.append(single[(k2 << 2) | (win >> 30)])
                        win = (win << bin(k2).count("1")) & 0xffffffff
                    win2, b = win0, []
                    for i in range(SPL // 2):
                        k4 = (kmask >> (4 * i)) & 15
                        b.extend(pairs[(k4 << 4) | (win2 >> 28)])
                        win2 = (win2 << bin(k4).count("1")) & 0xffffffff
                    assert a == b and win == win2, (ph, lo, hi, hex(win0))
                    assert bin(kmask).count("1") <= 24                 # the window is long enough: at most 24 of its 32 bits are consumed, and a key reads four
                    n += 1
    print(f"rate {cr}: {n} chains")
