"""The float64 resampler reference of tests/rxref.py, pinned to the oracle (oracle/o_resample.c) before tests/test_gpu_resampler.py lets it judge the
kernel: the design tap by tap, the stream output by output under the derived float32 bound, the call rule against the contract walked output by output, and
the support rule of ResamplerDesign::build against the table of ratios the GPU tests take their edge cases from."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rxref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(64, 70), (70, 64), (1, 1), (1, 2), (2, 1), (3, 2), (2, 5), (5, 13), (93, 1), (93, 92)]
IDS = [f"{i}-{d}" for i, d in RATIOS]


@pytest.mark.parametrize("interp,decim", RATIOS, ids=IDS)
def test_design_matches_oracle(po, interp, decim):
    """the oracle rounds to float three times (the window, the windowed sinc, the normalised tap): 4 * 2^-24 of the largest tap, per tap"""
    t32, ri, rd = po.resampler_taps(interp, decim)
    t64, ri64, rd64, nt = rxref.resampler_design64(interp, decim)
    assert (ri64, rd64) == (ri, rd) and len(t64) == len(t32) and nt == -(-len(t32) // ri)
    assert np.gcd(ri, rd) == 1 and ri * decim == rd * interp
    err = np.abs(t32.astype(np.float64) - t64)
    print(f"\n[design {interp}/{decim}] {len(t32)} taps, {ri} branches of {nt}: worst tap error {err.max() / (2.0 ** -24 * np.abs(t64).max()):.2f} x 2^-24 max|tap|")
    assert (err <= 4 * 2.0 ** -24 * np.abs(t64).max()).all()


@pytest.mark.parametrize("interp,decim", RATIOS, ids=IDS)
def test_stream_matches_oracle(po, interp, decim):
    """5000 Gaussian samples, scale 0.37: the oracle's sequential float32 sums against resample64 over the oracle's own taps, per output and per
    component under resample_bound"""
    rng = np.random.RandomState(11)
    x = (rng.randn(5000) + 1j * rng.randn(5000)).astype(np.complex64)
    t32, ri, rd = po.resampler_taps(interp, decim)
    nt = -(-len(t32) // ri)
    got = po.resample(x, interp, decim, 0.37)
    ref, a_re, a_im = rxref.resample64(x, t32, ri, rd, float(np.float32(0.37)))
    assert len(got) == len(ref) == -(-5000 * ri // rd)
    q_re = np.abs(got.real.astype(np.float64) - ref.real) / rxref.resample_bound(a_re, nt)
    q_im = np.abs(got.imag.astype(np.float64) - ref.imag) / rxref.resample_bound(a_im, nt)
    print(f"\n[oracle {interp}/{decim}] worst error / bound {max(q_re.max(), q_im.max()):.3f}")
    assert (q_re <= 1.0).all() and (q_im <= 1.0).all()


def test_resample64_is_the_definition():
    """the branch-by-branch evaluation against the sum of its docstring written out output by output"""
    rng = np.random.RandomState(5)
    x = rng.randn(97) + 1j * rng.randn(97)
    for ri, rd, ntaps in ((3, 2, 17), (2, 5, 11), (7, 1, 20), (1, 1, 5)):
        taps = rng.randn(ntaps)
        nt = -(-ntaps // ri)
        out, a_re, a_im = rxref.resample64(x, taps, ri, rd, -0.3)
        assert len(out) == -(-len(x) * ri // rd)
        for M in range(len(out)):
            n, b = M * rd // ri, M * rd % ri
            s, sr, si = 0j, 0.0, 0.0
            for k in range(nt):
                t = taps[b + k * ri] if b + k * ri < ntaps else 0.0
                v = x[n - k] if 0 <= n - k < len(x) else 0j
                s += t * v
                sr += abs(t) * abs(v.real)
                si += abs(t) * abs(v.imag)
            assert abs(out[M] - (-0.3) * s) <= 1e-13 * (sr + si) and abs(a_re[M] - 0.3 * sr) <= 1e-13 * sr and abs(a_im[M] - 0.3 * si) <= 1e-13 * si


@pytest.mark.parametrize("ri,rd", [(32, 35), (35, 32), (1, 1), (1, 2), (2, 1), (5, 13), (93, 1)])
def test_call_rule_counts_the_ready_outputs(ri, rd):
    """resampler_call_count against the contract walked one output at a time: output M is ready once input floor(M rd / ri) has been offered.  The
    stream position moves as any conforming block may move it: a call consumes between nothing and all it was offered, never past the newest input
    of the next output"""
    rng = np.random.RandomState(ri * 100 + rd)
    produced = consumed = 0
    for _ in range(400):
        nout, nin = int(rng.choice([1, 2, 7, 256, 1000])), int(rng.choice([1, 2, 3, 36, 500]))
        i = 0
        while i < nout and (produced + i) * rd // ri < consumed + nin:
            i += 1
        assert rxref.resampler_call_count(ri, rd, produced, consumed, nout, nin) == i
        produced += i
        consumed = int(rng.randint(consumed, min(consumed + nin, produced * rd // ri) + 1))
    assert rxref.resampler_call_count(ri, rd, 0, 0, 0, 5) == 0 and rxref.resampler_call_count(ri, rd, 0, 0, 5, 0) == 0


def _constant(name):
    src = open(os.path.join(ROOT, "gr_dvbt_amd", "csrc", "k_resample.hpp")).read()
    m = re.search(r"constexpr int %s = ([0-9 *]+);" % name, src)
    return int(np.prod([int(f) for f in m.group(1).split("*")]))


ACCEPTED = {(2, 5): (83, 725, None), (5, 13): (86, 753, None), (93, 1): (33, None, 3069)}        # nt, tile fill, ri * nt
REFUSED = {(94, 1): (None, 3102), (3, 8): (772, None), (35, 93): (770, None), (1, 93): (None, None)}


def test_support_table():
    """which ratios ResamplerDesign::build admits: ri * nt <= RS_MAX_BRANCH_FLOATS and 256 * rd / ri + nt + 2 <= RS_TILE_IN, computed here from the
    float64 design and the kernel's two constants"""
    assert _constant("RS_MAX_BRANCH_FLOATS") == rxref.RS_MAX_BRANCH_FLOATS == 3072 and _constant("RS_TILE_IN") == rxref.RS_TILE_IN == 768
    for i, d in RATIOS:
        _, ri, rd, nt = rxref.resampler_design64(i, d)
        assert rxref.resampler_supported(ri, rd, nt), (i, d)
    for (i, d), (nt_want, fill, table) in ACCEPTED.items():
        _, ri, rd, nt = rxref.resampler_design64(i, d)
        assert (ri, rd) == (i, d) and nt == nt_want and rxref.resampler_supported(ri, rd, nt)
        assert fill is None or 256 * rd // ri + nt + 2 == fill <= 768
        assert table is None or ri * nt == table <= 3072
    for (i, d), (fill, table) in REFUSED.items():
        _, ri, rd, nt = rxref.resampler_design64(i, d)
        assert (ri, rd) == (i, d) and not rxref.resampler_supported(ri, rd, nt)
        assert fill is None or 256 * rd // ri + nt + 2 == fill > 768
        assert table is None or ri * nt == table > 3072


@pytest.mark.parametrize("interp,decim", RATIOS, ids=IDS)
def test_kernel_tile_arithmetic_fits(interp, decim):
    """resample_scale_kernel's staging arithmetic restated (k_resample.hpp): a workgroup of outputs Mf .. Ml stages the inputs n_lo = floor(Mf rd / ri)
    - (nt - 1) .. n_hi = floor(Ml rd / ri) into s_x[RS_TILE_IN], and output M reads s_x[floor(M rd / ri) - n_lo - k], k = 0 .. nt - 1, and
    s_br[((M rd) mod ri) nt + k].  For every launch start M0 of one period of the branch counter and a few far ones, and launches of one partial, one
    full and several workgroups: every index inside its array, and the support rule's tile fill not below the widest span"""
    _, ri, rd, nt = rxref.resampler_design64(interp, decim)
    fill = 256 * rd // ri + nt + 2
    widest = 0
    for M0 in list(range(ri)) + [255, 256, 10 ** 6 + 1, 2 ** 33 + 5, 2 ** 40 - 1]:
        for count in (1, 255, 256, 257, 513):
            for m_blk in range(0, count, 256):
                Mf, Ml = M0 + m_blk, M0 + min(m_blk + 255, count - 1)
                n_lo, n_hi = Mf * rd // ri - (nt - 1), Ml * rd // ri
                span = n_hi - n_lo + 1
                M = np.arange(Mf, Ml + 1, dtype=np.int64)
                base = M * rd // ri - n_lo
                assert 0 < span <= rxref.RS_TILE_IN and (base - (nt - 1) >= 0).all() and (base < span).all()
                assert ((M * rd % ri) * nt + nt - 1 < ri * nt).all() and ri * nt <= rxref.RS_MAX_BRANCH_FLOATS
                widest = max(widest, span)
    print(f"\n[tile {interp}/{decim}] widest span {widest} of {rxref.RS_TILE_IN}, support rule's fill {fill}")
    assert widest <= fill
