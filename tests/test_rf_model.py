"""The RF front-end block's model (tests/rfref.py) against what it claims: a deterministic, stratified tone table whose power is the mask's integral for every
number of tones, a Rapp amplifier that is linear when small, saturates below A and never overflows, an IQ imbalance with the image where the theory puts
it, the identity with every stage off, and the stated order of the stages."""
import math

import numpy as np
import pytest

import chanref
import fadingref
import rfref as rr

MASK_10 = ((100.0, -60.0), (1e3, -70.0), (1e4, -80.0), (1e5, -100.0), (1e6, -120.0))     # its first two segments fall by 10 dB per decade: s = -1
MASK_OTHER = ((250.0, -55.0), (3e3, -81.0), (7e4, -96.0), (2.5e6, -131.0))               # no segment does


def test_the_table_is_deterministic_and_depends_on_the_seed():
    a = rr.tones(MASK_10, 32, seed=7)
    b = rr.tones(MASK_10, 32, seed=7)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    c = rr.tones(MASK_10, 32, seed=8)
    assert all(x != y for x, y in zip(a[1], c[1])) and a[0] != c[0]
    assert np.array_equal(a[2], c[2])                                          # the amplitudes belong to the strata, not to the draw
    assert len(set(a[1])) == 32 and len(set(a[0])) == 32
    assert rr.tones(MASK_10, 32, seed=7 + 2 ** 32)[1] != a[1]                  # the high half of the seed is part of the key
    assert all(0 < v < 2 ** 63 for v in a[0]) and all(0 <= v < 2 ** 64 for v in a[1])


def test_the_tagged_counter_is_neither_the_noises_nor_the_fading_tables():
    assert rr.TAG == 0x5246504E and rr.TAG != fadingref.TAG and rr.TAG != 0
    for seed in (0, 7, 2 ** 63 + 5):
        key = (seed & 0xffffffff, seed >> 32)
        for m in (0, 3, 31):
            tagged = chanref.philox4x32((m, 0, 0, rr.TAG), key).reshape(4)
            assert not (tagged == chanref.philox4x32((m, 0, 0, 0), key).reshape(4)).any()
            assert not (tagged == chanref.philox4x32((m, 0, 0, fadingref.TAG), key).reshape(4)).any()


@pytest.mark.parametrize("mask", [MASK_10, MASK_OTHER], ids=["with_-10dB_per_decade", "without"])
@pytest.mark.parametrize("M", [1, 8, 32])
def test_every_tone_lies_inside_its_stratum(mask, M):
    for seed in (0, 5, 2 ** 64 - 1):
        e = rr.edges(mask, M)
        assert e[0] == mask[0][0] and e[-1] == mask[-1][0] and all(a < b for a, b in zip(e, e[1:]))
        f = rr.tone_freqs(mask, M, seed)
        assert all(e[m] < f[m] < e[m + 1] for m in range(M))
        inc = rr.tones(mask, M, seed)[0]
        assert all(abs(inc[m] / 2.0 ** 64 * rr.SAMPLE_RATE - f[m]) <= 1e-12 * f[m] for m in range(M))


def _numeric_integral(mask, lo, hi, n=200001):
    """Simpson's rule on the log axis, segment by segment (the integrand has a kink at every mask point)"""
    total = 0.0
    for (fa, _), (fb, _) in zip(mask[:-1], mask[1:]):
        a, b = max(lo, fa), min(hi, fb)
        if b > a:
            t = np.linspace(math.log(a), math.log(b), n)
            y = rr.mask_level(mask, np.exp(t)) * np.exp(t)
            h = (t[-1] - t[0]) / (n - 1)
            total += h / 3.0 * (y[0] + y[-1] + 4.0 * y[1:-1:2].sum() + 2.0 * y[2:-1:2].sum())
    return total


@pytest.mark.parametrize("mask", [MASK_10, MASK_OTHER], ids=["with_-10dB_per_decade", "without"])
def test_the_tones_power_is_the_masks_integral_for_every_count(mask):
    whole = rr.mask_integral(mask, mask[0][0], mask[-1][0])
    num = _numeric_integral(mask, mask[0][0], mask[-1][0])
    print("closed form / numerical integral - 1:", whole / num - 1.0)
    assert abs(whole / num - 1.0) <= 1e-9
    for M in (1, 8, 32):
        e = rr.edges(mask, M)
        B = [rr.mask_integral(mask, e[m], e[m + 1]) for m in range(M)]
        power = sum((2.0 * math.sqrt(b)) ** 2 / 2.0 for b in B)                # sum a_m^2 / 2 in double, before the amplitudes are rounded to float32
        print(M, "sum a^2 / 2 over 2 integral L - 1:", power / (2.0 * whole) - 1.0)
        assert abs(power / (2.0 * whole) - 1.0) <= 1e-12
        amp = rr.tones(mask, M, 3)[2].astype(np.float64)
        assert abs((amp ** 2).sum() / 2.0 / (2.0 * whole) - 1.0) <= 2e-7        # and behind the rounding
    # the slope -1 is met exactly and nearly: the closed form is continuous there
    two = ((100.0, -60.0), (1000.0, -70.0))
    near = ((100.0, -60.0), (1000.0, -70.0 + 1e-8))
    assert abs(rr.mask_integral(two, 100.0, 1000.0) - 1e-6 * 100.0 * math.log(10.0)) <= 1e-18
    assert abs(rr.mask_integral(near, 100.0, 1000.0) / rr.mask_integral(two, 100.0, 1000.0) - 1.0) <= 1e-8


def test_the_amplifier():
    A = 0.37
    ang = np.exp(1j * np.linspace(-3.0, 3.0, 7))
    for p in (0.5, 1.0, 2.0, 16.0):
        # linear where small: at |x| = 1e-3 A the gain is 1 - 1e-6p / (2p), which is 1 to 1e-12 from p = 2 on (2.5e-13) and 1 - 5e-7 at p = 1
        small = 1e-3 * A * ang
        if p >= 2.0:
            assert np.abs(rr.pa(small, A, p) / small - 1.0).max() <= 1e-12
        if p >= 1.0:
            assert np.abs(rr.pa(small, A, p) / small - (1.0 - 1e-6 ** p / (2.0 * p))).max() <= 1e-12
        # |u| < A always, and growing with |x|: strictly where float64 can tell 1 - (|x| / A)^(-2p) / (2p) from 1, to a rounding beyond
        r = np.concatenate([np.linspace(0.0, 2.0 * A, 2001), A * np.logspace(0.31, 30.0, 500)])
        u = rr.pa(r.astype(np.complex128), A, p)
        assert (np.abs(u)[:2001] < A).all() and (np.diff(np.abs(u)[:2001]) > 0).all()
        assert (np.abs(u) <= A * (1.0 + 4e-16)).all() and (np.diff(np.abs(u)) >= -4e-16 * A).all()
        # the 3 dB point of the smooth knee
        assert abs(abs(rr.pa(np.array([A * ang[2]]), A, p)[0]) - 2.0 ** (-1.0 / (2.0 * p)) * A) <= 1e-15
        # the phase is preserved
        x = np.outer(np.array([1e-3, 0.5, 1.0, 2.0, 1000.0]) * A, ang).reshape(-1)
        y = rr.pa(x, A, p)
        assert np.abs(np.angle(y * np.conj(x))).max() <= 1e-15
        # both forms are the definition where the definition does not overflow
        t = (np.abs(x) / A) ** 2
        assert np.abs(y - x * (1.0 + t ** p) ** (-1.0 / (2.0 * p))).max() <= 1e-15 * A
    with np.errstate(over="raise", invalid="raise", divide="raise"):          # no overflow, no invalid operation (t^(-p) may underflow to 0: that is its value)
        far = rr.pa(np.array([1000.0 * A * ang[1], 1e30 * ang[4], 3e38 + 3e38j]), A, 16.0)
    assert np.isfinite(far).all() and np.abs(np.abs(far) / A - 1.0).max() <= 1e-15       # |u| -> A
    assert rr.pa(np.zeros(3, np.complex64), A, 16.0).tolist() == [0, 0, 0]
    assert rr.pa(np.array([1 + 2j]), 0.0).tolist() == [1 + 2j]                 # A == 0: off
    assert np.array_equal(rr.pa(np.array([0.3 - 0.1j]), A, 0.0), rr.pa(np.array([0.3 - 0.1j]), A, 2.0))   # p == 0 stands for 2


def test_iq_imbalance_puts_the_image_where_the_theory_does():
    N, k = 4096, 37
    x = np.exp(2j * np.pi * k * np.arange(N) / N)
    mu, nu = rr.iq_imbalance(0.5, 3.0)
    X = np.fft.fft(rr.iq(x, mu, nu)) / N
    direct, image = abs(X[k]) ** 2, abs(X[N - k]) ** 2
    assert abs(image / direct - abs(nu) ** 2 / abs(mu) ** 2) <= 1e-12
    others = np.delete(np.abs(X), [k, N - k])
    assert others.max() <= 1e-12
    assert abs(rr.irr_db(mu, nu) - 28.2) <= 0.05
    assert abs(rr.irr_db(*rr.iq_imbalance(0.2, 1.0)) - 36.8) <= 0.05
    assert rr.iq_imbalance(0.0, 0.0) == (1.0, 0.0)
    # the helper is a real gain and phase error of the Q arm: I is untouched
    g, psi = 10 ** (0.5 / 20), math.radians(3.0)
    z = 0.3 - 0.8j
    v = rr.iq(np.array([z]), mu, nu)[0]
    assert abs(v.real - z.real) <= 1e-15 and abs(v.imag - g * (z.imag * math.cos(psi) - z.real * math.sin(psi))) <= 1e-15


def test_all_stages_off_is_the_identity():
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(100) + 1j * rng.standard_normal(100)).astype(np.complex64)
    assert np.array_equal(rr.rf(x, rr.params(), 12345), x)
    assert np.array_equal(rr.rf(x, rr.params(mu=0), 0), x)                     # a zeroed struct's mu stands for 1
    assert rr.params(smoothness=0.0).smoothness == 2.0


def test_the_stages_run_in_the_stated_order():
    rng = np.random.default_rng(3)
    x = 0.5 * (rng.standard_normal(64) + 1j * rng.standard_normal(64))
    first = 2 ** 40 + 3
    t = rr.tones(MASK_10, 4, seed=1)
    t = (t[0], t[1], t[2] * 30.0)                                              # loud enough to matter
    mu, nu = rr.iq_imbalance(0.5, 3.0)
    A, dc = 0.6, 0.05 - 0.02j
    full = rr.rf(x, rr.params(A, 2.0, t, mu, nu, dc), first)
    mu, nu = complex(np.complex64(mu)), complex(np.complex64(nu))
    dc, A = complex(np.complex64(dc)), float(np.float32(A))
    rot = np.exp(1j * rr.phi((t[0], t[1], t[2].astype(np.float32)), first, 64))
    u = x * (1.0 + (np.abs(x) / A) ** 4) ** -0.25
    want = mu * (u * rot) + nu * np.conj(u * rot) + dc
    assert np.abs(full - want).max() <= 1e-15
    # every swap of two neighbouring stages is another function
    pa_after_pn = rr.pa(x * rot, A)                                            # commutes: the amplifier does not see the phase ...
    assert np.abs(pa_after_pn - u * rot).max() <= 1e-15
    iq_first = rr.iq(x, mu, nu)                                                # ... but it does see the IQ imbalance and the DC
    assert np.abs((mu * rr.pa(iq_first, A) * rot + dc) - full).max() > 1e-3
    assert np.abs((mu * (u * rot + dc) + nu * np.conj(u * rot + dc)) - full).max() > 1e-4       # DC in front of the IQ stage
    assert np.abs(((mu * u + nu * np.conj(u)) * rot + dc) - full).max() > 1e-4                  # IQ in front of the phase noise: the image turns the other way
    assert np.abs(rr.pa(x + dc, A) - (u + dc)).max() > 1e-3                                      # DC in front of the amplifier


def test_phases_are_exact_far_into_the_stream():
    t = rr.tones(MASK_10, 8, seed=9)
    far = 2 ** 40 + 3
    a = rr.phi(t, far, 50)
    want = np.zeros(50)
    for inc, ph, amp in zip(*t):
        th = np.array([(((ph + inc * (far + i)) % 2 ** 64) >> 32) / 2.0 ** 32 for i in range(50)])   # Python integers
        want = want + float(amp) * np.sin(2 * np.pi * th)
    assert np.array_equal(a, want)
    assert abs(rr.rms_deg(rr.tones(MASK_10, 32, 0)) - 1.9) <= 0.06
    assert abs(rr.rms_deg(rr.tones(tuple((f, d - 10.0) for f, d in MASK_10), 32, 0)) - 0.6) <= 0.02
