"""The Viterbi decoder's one branch-metric permute per step (gr_dvbt_amd/csrc/k_viterbi3.hpp: v3_init_lane's selectors, v3_step), restated in numpy; no GPU needed.

A lane holds four cells (r = register 0/1, h = half 0/1) of index c = r:h:a, a = v3_log(lane); at phase P the cell holds state rotl6(c, P) and its label class -- the byte of the
step word its delta comes from -- is a function of the state's bits 0, 1, 2 and 4.  v3_step builds F = v_perm_b32(0, W, sel[P]) = [0, byte, 0, byte'] once per step:
 * at the phases 0, 2, 3, 4 the two bytes are the classes of register 0's two halves, and register 1 takes the same word (phases 0, 4) or its negative (2, 3);
 * at the phases 1 and 5 a register's two halves share their class (cell bit 4 sits on state bit 5 or 3, which no parity tap reads), so the two bytes are the classes of
   register 0 and of register 1, and the packed adds take their half of F through the op_sel of the VOP3P encoding (register 0: the low half into both lanes of the add,
   register 1: the high half).
Checked here for every lane, register, half and every step word of the 16-entry table: the delta a cell receives is the delta of its own label class, and the path-byte
position below it receives zero.  And that the trick stops at two phases: at the other four the halves of a register do not share their class."""
import numpy as np
import pytest


def rotl6(c, p):
    return ((c << p) | (c >> (6 - p))) & 63


def v3_log(p):
    q = p & 7
    a2 = (q >> 2) & 1
    return (p & 8) | (a2 << 2) | ((q ^ (7 if a2 else 0)) & 3)


def label_class(P, r, h, a):
    """v3_init_lane's idx[h]: c0 | c1 << 1 of the butterfly the cell's state belongs to"""
    i = rotl6((r << 5) | (h << 4) | a, P) & 31
    c0 = ((i >> 2) ^ (i >> 1) ^ i) & 1
    c1 = ((i >> 4) ^ (i >> 2) ^ (i >> 1)) & 1
    return c0 | (c1 << 1)


def selector(P, a):
    """v3_init_lane's sel[P]: the classes of register 0's halves, or at the phases 1 and 5 of the two registers"""
    if P in (1, 5):
        lo, hi = label_class(P, 0, 0, a), label_class(P, 1, 0, a)
    else:
        lo, hi = label_class(P, 0, 0, a), label_class(P, 0, 1, a)
    return 0x0c | (lo << 8) | (0x0c << 16) | (hi << 24)


def v_perm_b32(s0, s1, sel):
    """byte i of the result = byte sel[i] of the eight bytes s0:s1 (0..3 = s1), 0x0c = the constant 0"""
    out = 0
    for i in range(4):
        s = (sel >> (8 * i)) & 0xff
        assert s == 0x0c or s < 8
        b = 0 if s == 0x0c else (((s0 << 32) | s1) >> (8 * s)) & 0xff
        out |= b << (8 * i)
    return out


def step_words():
    """v3_init_lut's sixteen words: four class deltas, doubled, one per byte"""
    words = []
    for e in range(16):
        k0, k1, t1, t0 = (e >> 2) & 1, (e >> 3) & 1, (e >> 1) & 1, e & 1
        u0 = 1 - 2 * t1 if k0 else 0
        u1 = (1 - 2 * (t0 if k0 else t1)) if k1 else 0
        d = [2 * (u0 + u1), 2 * (-u0 + u1), 2 * (u0 - u1), 2 * (-u0 - u1)]
        words.append(sum((x & 0xff) << (8 * i) for i, x in enumerate(d)))
    return words


WORDS = step_words()
LANES = [v3_log(pl) for pl in range(16)]


def s8(x):
    return x - 256 if x >= 128 else x


def s16(x):
    return x - 65536 if x >= 32768 else x


def test_lanes_are_the_sixteen_cell_indices():
    assert sorted(LANES) == list(range(16))


@pytest.mark.parametrize("P", [1, 5])
def test_one_permute_delivers_every_cells_delta(P):
    """op_sel:[0,r] op_sel_hi:[1,r] on the second source: both halves of register r's add read half r of F"""
    for a in LANES:
        sel = selector(P, a)
        for W in WORDS:
            F = v_perm_b32(0, W, sel)
            for r in range(2):
                half = (F >> (16 * r)) & 0xffff
                for h in range(2):
                    want = s8((W >> (8 * label_class(P, r, h, a))) & 0xff)
                    assert half & 0xff == 0, (P, a, r, h, hex(F))                       # the path byte receives a zero delta
                    assert s16(half) == want * 256, (P, a, r, h, hex(W), hex(F))       # the metric field (bits 15:8) the delta of the cell's own class


@pytest.mark.parametrize("P", [1, 5])
def test_halves_share_the_class_and_registers_differ_by_a_constant(P):
    for a in LANES:
        for r in range(2):
            assert label_class(P, r, 0, a) == label_class(P, r, 1, a)
        assert label_class(P, 1, 0, a) ^ label_class(P, 0, 0, a) == {1: 1, 5: 2}[P]


@pytest.mark.parametrize("P", [0, 2, 3, 4])
def test_the_other_phases_need_both_halves_classes(P):
    """the halves of a register do not share their class there -- in no lane, in fact -- so the selector's two bytes are taken by the halves and register 1 lives on
    register 0's word: the same deltas (class xor 0) or the negated ones (class xor 3)"""
    differ = [label_class(P, r, 0, a) != label_class(P, r, 1, a) for a in LANES for r in range(2)]
    assert all(differ)
    for a in LANES:
        sel = selector(P, a)
        for h in range(2):
            assert label_class(P, 1, h, a) ^ label_class(P, 0, h, a) == {0: 0, 2: 3, 3: 3, 4: 0}[P]
        for W in WORDS:
            F = v_perm_b32(0, W, sel)
            for h in range(2):
                half = (F >> (16 * h)) & 0xffff
                d0 = s8((W >> (8 * label_class(P, 0, h, a))) & 0xff)
                d1 = s8((W >> (8 * label_class(P, 1, h, a))) & 0xff)
                assert half & 0xff == 0 and s16(half) == d0 * 256
                assert d1 == (d0 if P in (0, 4) else -d0)


def test_class_difference_of_the_registers_by_phase():
    assert [label_class(P, 1, 0, 0) ^ label_class(P, 0, 0, 0) for P in range(6)] == [0, 1, 3, 3, 0, 2]
    assert np.all([[label_class(P, 1, h, a) ^ label_class(P, 0, h, a) == (0, 1, 3, 3, 0, 2)[P] for a in LANES for h in range(2)] for P in range(6)])
