"""The block bounds of staging's loads (gr_dvbt_amd/csrc/k_viterbi3.hpp, v3_decode: l_first / l_last), restated beside the per-lane test they replace.

A decoder (one row of 16 lanes) stages block jb of 24 windows from the input byte y(jb) = rb(2 t) / m, t = max(tb0 + 8 jb, 0), rb(p) = (p / plen) n + pfx(p % plen);
its lanes pl < nload read 16 bytes each from src = y - off + 16 pl, off = (in + y - in_base) & 3.  The per-lane test, which stays on the path outside the bounds, is
    src >= in_base && src + 16 <= n_in_bytes            for every pl < nload;
the bounds call the blocks l_first <= jb <= l_last safe, from two thresholds on y that are inverted through rb in whole puncture periods and one magic division (VitParams.magic_n).
Checked here, in exact integers, for five rates x three constellations, streams of 1 to 4 chunks plus a ragged tail (and streams shorter than a chunk), the pointer `in` at
byte offsets 0..3, in_base 0..3 and in the middle of the stream (a later call of the single block: the input in front of in_base is gone, the first decoders' warm-up reaches
in front of it), first chunks whose warm-up reaches in front of the stream:
 * every block the bounds call safe is safe for every lane -- per decoder, and for the wavefront's bounds (max / min over its four rows, a row without a decoder not counting);
 * a decoder's safe blocks are one run, and the bounds miss at most its first and its last block (the inversion rounds to a whole puncture period, up to seven steps, on the
   safe side: less than a window); where `in` is aligned, in_base = 0 and the stream goes on behind the decoder, no block is missed at all."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_viterbi_shortcut_model import NTB, PUNCT  # noqa: E402

BLK, WARM, B = 24, 72, 264
M_OF_CONST = (2, 4, 6)
MAGIC = lambda d: (2 ** 64 - 1) // d + 1  # noqa: E731


def _umulhi(a, b):
    assert 0 <= a < 2 ** 64 and 0 <= b < 2 ** 64
    return (a * b) >> 64


class Dec:
    def __init__(self, cr, m, b0, total_steps, in_base, a):
        p = PUNCT[cr]
        self.m, self.n, self.plen, self.p, self.ntb = m, sum(p), len(p), p, NTB[cr]
        self.total_out = total_steps // 8 - self.ntb
        self.active = b0 < self.total_out
        self.J = -(-(WARM + B + self.ntb - 1) // BLK) * BLK
        self.tb0 = 8 * (b0 + 2 - WARM - 1) - 2
        self.n_in_bytes = (total_steps * 2 // self.plen * self.n + m - 1) // m
        self.nload = ((384 + 2 * m - 2) // m + 3 + 15) // 16
        self.in_base, self.a = in_base, a

    def y(self, jb):
        pbit = 2 * max(self.tb0 + 8 * jb, 0)
        pq, ph = divmod(pbit, self.plen)
        return (pq * self.n + sum(self.p[:ph])) // self.m

    def lanes_safe(self, jb):
        """the per-lane test of the byte-wise path, for every loading lane"""
        y = self.y(jb)
        off = (self.a + y - self.in_base) & 3
        return all(y - off + 16 * pl >= self.in_base and y - off + 16 * pl + 16 <= self.n_in_bytes for pl in range(self.nload))

    def bounds(self):
        """(first, last) as v3_decode forms them, line by line"""
        a, m, J = self.a, self.m, self.J
        if not self.active:
            return 0, J
        H = self.n_in_bytes - self.in_base + a - 16 * self.nload
        r_lo = (self.in_base + ((4 - a) & 3)) * m
        r_hi = (self.in_base + (H & ~3) + 3 - a + 1) * m - 1
        first, last = 0, J
        if r_lo > 0:
            p = (_umulhi(r_lo - 1, MAGIC(self.n)) + 1) * self.plen
            w = (((p + 1) >> 1) - self.tb0 + 7) >> 3
            first = 0 if w <= 0 else J if w >= J else (w + BLK - 1) // BLK * BLK
        if H < 0 or r_hi < 0:
            last = -1
        else:
            p = _umulhi(r_hi, MAGIC(self.n)) * self.plen
            w = ((p >> 1) - self.tb0) >> 3
            last = -1 if w < 0 else J if w >= J else w // BLK * BLK
        return first, last


def _streams(cr):
    """total trellis steps: whole bytes, 1 to 4 chunks plus a ragged tail, and two streams shorter than a chunk"""
    ntb = NTB[cr]
    return [8 * (nbytes + ntb) for nbytes in (30, 200, B + 5, 2 * B + 131, 3 * B + 1, 4 * B + 77, 4 * B + 263)]


@pytest.mark.parametrize("cr", range(5))
@pytest.mark.parametrize("const", range(3))
def test_bounds_are_safe_and_miss_only_the_ends(cr, const):
    m = M_OF_CONST[const]
    ndec = missed_total = safe_total = 0
    for total_steps in _streams(cr):
        total_out = total_steps // 8 - NTB[cr]
        nch = -(-total_out // B)
        for a in range(4):
            for in_base in (0, 1, 2, 3, 150, 151, 301):
                decs = [Dec(cr, m, c * B, total_steps, in_base, a) for c in range(4 * -(-nch // 4))]
                for d in decs:
                    if not d.active:
                        continue
                    ndec += 1
                    blocks = list(range(0, d.J, BLK))
                    truth = [jb for jb in blocks if d.lanes_safe(jb)]
                    first, last = d.bounds()
                    called = [jb for jb in blocks if first <= jb <= last]
                    assert set(called) <= set(truth), (total_steps, a, in_base, d.tb0, first, last, truth)
                    assert truth == blocks[blocks.index(truth[0]):blocks.index(truth[-1]) + 1] if truth else True      # one run
                    missed = sorted(set(truth) - set(called))
                    assert len(missed) <= 2 and set(missed) <= ({truth[0], truth[-1]} if truth else set()), (total_steps, a, in_base, d.tb0, first, last, truth)
                    if a == 0 and in_base == 0 and d.y(d.J) + 16 * d.nload + 3 <= d.n_in_bytes:
                        assert called == blocks                                                                   # the decoders in the middle of a stream: every block
                    missed_total += len(missed)
                    safe_total += len(truth)
                # the wavefront's bounds: max / min over its four rows
                for w0 in range(0, len(decs), 4):
                    bs = [d.bounds() for d in decs[w0:w0 + 4]]
                    first, last = max(b[0] for b in bs), min(b[1] for b in bs)
                    for d in decs[w0:w0 + 4]:
                        if d.active:
                            assert all(d.lanes_safe(jb) for jb in range(0, d.J, BLK) if first <= jb <= last)
    print(f"rate {cr} m {m}: {ndec} decoders, {safe_total} safe blocks, {missed_total} of them missed by the bounds")
    assert ndec > 0 and safe_total > 0
