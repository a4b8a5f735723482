"""The sample-clock offset block's numpy model tests/clockref.py: against the oracle's resampler po.clock_offset, and against its own definition (positions are
Python ints, f == 0 copies, a stream may be cut anywhere).

TOL: 1e-5 of the model's peak sample, the project's bound for a float32 baseband (test_gpu_tx._close).  The oracle rounds its coefficients to float32 and
computes its positions in double: its distance from the model is a few 1e-7 of the peak.
"""
import numpy as np
import pytest

import clockref

FAR = 2 ** 40 + 3


def _within_tol(got, model):
    assert got.shape == model.shape and len(model) > 0
    err, peak = np.abs(got - model).max(), np.abs(model).max()
    print(f"\nlargest error {err:.3e} = {err / peak:.2e} of the peak {peak:.4f}")
    assert err <= 1e-5 * peak


@pytest.fixture(scope="module")
def random_x():
    rng = np.random.RandomState(23)
    x = (rng.randn(200000) + 1j * rng.randn(200000)).astype(np.complex64)
    x[0] = complex(-0.0, 0.0)
    return x


@pytest.mark.parametrize("ppm", [10.0, -40.0, 55.0, 1000.0, -1000.0])
def test_model_against_the_oracles_resampler(po, random_x, ppm):
    ref = po.clock_offset(random_x, ppm)
    got = clockref.resample(random_x, ppm)
    n = min(len(ref), len(got))
    assert n > 0.99 * len(random_x) / (1 + ppm * 1e-6) - 20 and len(got) >= len(ref)        # the oracle trims a little more than the taps need
    assert len(got) == clockref.outputs(len(random_x), ppm, 8.0)
    _within_tol(got[:n], ref[:n].astype(np.complex128))


@pytest.mark.parametrize("taps", [16, 32, 64])
@pytest.mark.parametrize("start", [0.0, 5.0, None])
def test_a_whole_position_copies_the_sample_bit_for_bit(random_x, taps, start):
    x = random_x[:4097]
    H = taps // 2
    s = H if start is None else int(start)
    got = clockref.resample(x, 0.0, start=start, taps=taps)
    assert len(got) == len(x) - H - s
    assert got.astype(np.complex64).tobytes() == x[s:s + len(got)].tobytes()               # -0.0 at x[0] included (start = 0)
    # a whole position now and then: a step of 1 + 2^-10 puts every 1024th output on a sample
    ppm = 1e6 * 2.0 ** -10
    assert clockref.step(ppm) == 2 ** 64 + 2 ** 54
    got = clockref.resample(x, ppm, start=float(H), taps=taps)
    on = np.arange(0, len(got), 1024)
    assert len(on) >= 3
    for m in on:
        base, f = clockref.pos(m, ppm, H)
        assert f == 0 and got[m] == x[base] and np.signbit(got[m].real) == np.signbit(x[base].real)
    assert clockref.pos(1, ppm, H)[1] == 2 ** 54 and got[1] != x[H + 1]


@pytest.mark.parametrize("ppm", [37.5, -1000.0])
@pytest.mark.parametrize("start", [8.0, 8.5, 8 + 2.0 ** -40])
def test_positions_far_out_are_python_int_arithmetic(ppm, start):
    S = 2 ** 64 + round(ppm * 1e-6 * 2 ** 64)
    assert abs(clockref.step(ppm) - S) <= 4096                 # (the float product ppm 1e-6 is rounded once: the definition's S, not the ideal one)
    S = clockref.step(ppm)
    P0 = clockref.p0(start)
    assert P0 == int(start) * 2 ** 64 + int((start - int(start)) * 2 ** 64)
    for m in (0, 1, FAR, FAR + 1, 2 ** 48):
        P = P0 + m * S
        assert clockref.pos(m, ppm, start) == (P >> 64, P & (2 ** 64 - 1))
    # E is the smallest m whose support reaches N
    for N in (0, 7, 8, 9, 200, 2 ** 31 + 1, FAR, 2 ** 48 + 12345):
        m = clockref.E(N, ppm, start)
        assert m >= 0 and clockref.pos(m, ppm, start)[0] + 8 >= N
        assert m == 0 or clockref.pos(m - 1, ppm, start)[0] + 8 < N


@pytest.mark.parametrize("taps,ppm", [(16, 55.0), (64, -1000.0)])
def test_splits_and_pieces_commute(random_x, taps, ppm):
    x = random_x[:30001]
    H = taps // 2
    whole = clockref.resample(x, ppm, taps=taps)
    # counts: what calls of any sizes emit adds up to what one call emits
    total, seen = 0, 0
    for n in (1, 63, 1000, 0, 4097, len(x) - 5161):
        total += clockref.outputs(seen + n, ppm, H, taps) - clockref.outputs(seen, ppm, H, taps)
        seen += n
    assert seen == len(x) and total == len(whole)
    # a piece: outputs M.. from the inputs base(M) - (H - 1)..; the same values, not only close ones (the same taps enter the same sums)
    M = 10001
    fi = clockref.first_in_for(M, ppm, H, taps)
    piece = clockref.resample(x[fi:], ppm, taps=taps, first_out=M, first_in=fi)
    assert len(piece) == len(whole) - M and (piece == whole[M:]).all()
    # the same far out: numbering moved by FAR outputs and the inputs that belong to them
    fo = FAR
    fi_far = clockref.first_in_for(fo, ppm, H, taps)
    far = clockref.resample(x, ppm, taps=taps, first_out=fo, first_in=fi_far)
    assert len(far) == clockref.outputs(len(x), ppm, H, taps, fo, fi_far) > 0.99 * len(x) / (1 + ppm * 1e-6) - 2 * taps
    # an input that begins before what first_out needs: the outputs in front of first_out are not emitted
    early = clockref.resample(x, ppm, taps=taps, first_out=M, first_in=0)
    assert len(early) == len(whole) - M and (early == whole[M:]).all()
