"""The channel block's numpy model (tests/chanref.py) against published known answers of Philox4x32-10, recorded first noise samples, the statistics a unit
Gaussian must show, and -- for the echoes and the carrier offset -- the oracle's test channel po.channel.  No GPU."""
import numpy as np
import pytest

import chanref

SEEDS = (5, 0x0123456789abcdef)

# (counter, key) -> words: the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10) and one more with key (5, 0)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ((0, 0, 0, 0), (5, 0), (0xc417681d, 0x11d85194, 0xfbd62c3b, 0xf739e278)),
]


@pytest.mark.parametrize("counter,key,want", PHILOX_KAT)
def test_philox_known_answers(counter, key, want):
    got = chanref.philox4x32(counter, key).reshape(-1)
    assert [int(w) for w in got] == list(want), [hex(int(w)) for w in got]


def test_first_noise_samples():
    want = np.array([0.66127639 + 0.30968726j, 0.17690785 - 0.03869601j, 0.80873223 + 1.20894143j, 0.77005733 + 0.71815465j])
    got = chanref.noise(5, 0, 4)
    assert np.abs(got - want).max() < 1e-8, got
    want = np.array([0.08168965 + 1.28767798j, -0.65319043 - 1.04844336j, -1.4251775 - 0.48185339j, 0.94508081 + 0.21605066j])
    got = chanref.noise(5, 2 ** 40 + 3, 4)
    assert np.abs(got - want).max() < 1e-8, got


def test_noise_depends_on_seed_and_index_alone():
    a = chanref.noise(5, 0, 4099)
    b = np.concatenate([chanref.noise(5, 0, 1), chanref.noise(5, 1, 1000), chanref.noise(5, 1001, 3098)])
    assert a.tobytes() == b.tobytes()
    assert np.abs(chanref.noise(6, 0, 64) - a[:64]).min() > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_noise_statistics(seed):
    g = chanref.noise(seed, 0, 1 << 20)
    c = np.concatenate([g.real, g.imag])
    assert len(c) == 1 << 21
    figures = dict(mean=c.mean(), var=c.var(), m4=np.mean(c ** 4), peak=np.abs(c).max(), cross=np.mean(g.real * g.imag),
                   lag1=np.mean(c[:-1] * c[1:]) / c.var())
    print(hex(seed), figures)
    assert abs(figures["mean"]) < 0.005
    assert abs(figures["var"] - 1.0) < 0.005
    assert abs(figures["m4"] - 3.0) < 0.05
    assert figures["peak"] < 5.78
    assert abs(figures["cross"]) < 0.005
    assert abs(figures["lag1"]) < 0.005
    # per component and along the stream as well: neighbouring samples share a Philox block
    for v in (g.real, g.imag):
        assert abs(np.mean(v[:-1] * v[1:]) / v.var()) < 0.005


def test_phase_is_an_integer_product():
    inc = chanref.phase_inc(3.37, 2048)
    assert inc == int(round(3.37 / 2048 * 2.0 ** 64))
    assert chanref.phase_inc(-7.63, 2048) == 2 ** 64 - int(round(7.63 / 2048 * 2.0 ** 64))
    assert chanref.phase_inc(0.0, 0) == 0
    # a whole number of turns later the phasor is the same: nothing decays with n
    n = 2 ** 40 + 3
    a = chanref.phasor(1.0, 2048, n, 8)                       # inc = 2^53: period 2048 samples exactly
    b = chanref.phasor(1.0, 2048, n % 2048, 8)
    assert a.tobytes() == b.tobytes()


def test_deterministic_part_against_the_oracles_channel(po):
    c = po.cfg(po.QAM16, po.C1_2, po.T2k)
    iq = po.tx(c, po.make_ts(po.packets_per_superframe(c), 3), lead_in=1000, tail=3 * c.N)
    echoes = ((57, 0.15), (19, -0.1j))
    ref = po.channel(iq, c.N, cfo=3.37, echoes=echoes)
    got = chanref.channel(iq, echoes=echoes, cfo=3.37, fft_length=c.N)
    assert got.shape == ref.shape
    # po.channel returns complex64: its rounding is 6e-8 of a sample, the bound is 1e-9 of the peak -- compare in double, against the same arithmetic
    x = iq.astype(np.complex128)
    y = x.copy()
    for d, a in echoes:
        y[d:] += a * x[:-d]
    y *= np.exp(2j * np.pi * 3.37 / c.N * np.arange(len(x), dtype=np.float64))
    assert (y.astype(np.complex64) == ref).all()              # y is po.channel before its rounding
    peak = np.abs(y).max()
    assert np.abs(got - y).max() < 1e-9 * peak
    assert np.abs(got.astype(np.complex64) - ref).max() <= 1.2e-7 * peak


def test_splits_and_first_sample_commute_in_the_model():
    rng = np.random.RandomState(1)
    x = (rng.randn(3000) + 1j * rng.randn(3000)).astype(np.complex64)
    kw = dict(cfo=-7.63, fft_length=2048, noise_sigma=0.5, seed=5)
    whole = chanref.channel(x, **kw, first_sample=2 ** 40 + 3)
    tail = chanref.channel(x[1001:], **kw, first_sample=2 ** 40 + 3 + 1001)
    assert whole[1001:].tobytes() == tail.tobytes()
