"""CPU: the scanner's numpy model (tests/scanref.py) pinned on the oracle's modulator at every mode x guard -- the definitions of include/dvbt_hip.h's "scan"
block find FFT size, guard interval, symbol start and fractional carrier offset at 3 dB and at -3 dB, and read nothing into noise or a tone."""
import math
import numpy as np
import pytest

import scanref

LENGTH = 8 * 10240 + 9000
CUT = 777
# modulation, code rate, cfo, echo (delay as a function of the guard length, amplitude), SNR in dB
SETS = {"a": ("QAM64", "C7_8", 0.37, (lambda cp: cp // 2, 0.5j), 3.0),
        "b": ("QPSK", "C1_2", -0.45, (lambda cp: cp - 3, 0.9), -3.0)}


@pytest.fixture(scope="module")
def verdicts(po):
    """{(set, mode, guard): the float32 model's verdict} of the 16 streams, computed once"""
    out = {}
    for name, (con, rate, cfo, (delay, amp), snr) in SETS.items():
        for mode in (po.T2k, po.T8k):
            for guard in range(4):
                c = po.cfg(getattr(po, con), getattr(po, rate), mode, guard)
                iq = po.tx(c, po.make_ts(po.packets_per_superframe(c), 11), scale=1.0)
                iq = po.channel(iq, c.N, cfo=cfo, echoes=((delay(c.cp), amp),), snr_db=snr, seed=11)
                out[name, mode, guard] = scanref.scan(iq[CUT:CUT + LENGTH])
    return out


def test_every_mode_and_guard_is_detected_with_the_defaults(verdicts):
    worst_ratio, lowest_rho = math.inf, math.inf
    for (name, mode, guard), v in sorted(verdicts.items()):
        h = 4 * mode + guard
        ratio = v["rho"][h] / max(r for k, r in enumerate(v["rho"]) if k != h)
        print(f"set {name} mode {mode} guard {guard}: rho {v['rho'][h]:.4f}, best other {v['rho'][h] / ratio:.4f}, ratio {ratio:.3f}, "
              f"start {v['symbol_start'][h]}, cfo {v['cfo'][h]:+.4f}")
        worst_ratio, lowest_rho = min(worst_ratio, ratio), min(lowest_rho, v["rho"][h])
        assert (v["detected"], v["mode"], v["guard"]) == (1, mode, guard), (name, mode, guard, v["rho"])
    print(f"worst ratio of the true hypothesis to the best other {worst_ratio:.3f}, lowest true rho {lowest_rho:.4f}")


def test_carrier_offset_and_symbol_start_under_set_a(verdicts):
    for (name, mode, guard), v in verdicts.items():
        if name != "a":
            continue
        h = 4 * mode + guard
        _, G, S = scanref.dims(h)
        assert abs(v["cfo"][h] - 0.37) <= 0.01, (mode, guard, v["cfo"][h])
        d = (v["symbol_start"][h] - (-CUT) % S) % S
        assert min(d, S - d) <= G // 8, (mode, guard, v["symbol_start"][h], (-CUT) % S)


def _noise(n, seed):
    rng = np.random.RandomState(seed)
    return ((rng.randn(n) + 1j * rng.randn(n)) / np.sqrt(2.0)).astype(np.complex64)


def test_noise_alone_is_not_a_signal():
    v = scanref.scan(_noise(LENGTH, 1))
    print("noise: rho", [f"{r:.4f}" for r in v["rho"]])
    assert v["detected"] == 0 and v["mode"] == v["guard"] == -1


def test_a_tone_in_noise_is_not_a_signal():
    n = np.arange(LENGTH, dtype=np.float64)
    x = np.exp(2j * np.pi * 0.01234 * n) + 0.3 * _noise(LENGTH, 1).astype(np.complex128)
    v = scanref.scan(x.astype(np.complex64))
    print("tone: rho", [f"{r:.4f}" for r in v["rho"]])
    assert v["detected"] == 0


def test_one_sample_short_of_the_minimum_is_not_enough(verdicts, po):
    c = po.cfg(po.QAM64, po.C7_8, po.T2k, po.G1_8)
    iq = po.tx(c, po.make_ts(po.packets_per_superframe(c), 11), scale=1.0)
    assert scanref.scan(iq[:scanref.MIN_SAMPLES])["detected"] == 1
    v = scanref.scan(iq[:scanref.MIN_SAMPLES - 1])
    assert v["detected"] == 0 and v["symbols"][7] == 7 and max(v["rho"]) > 0.5


def test_float32_sums_stay_within_the_summation_bound(po):
    """per bin, |float32 model - float64 model| <= 20 2^-24 sum_j |a||b| (16 sequential additions plus the products' and the inner sum's roundings; the
    double additions are 2^-29 of that); for E, whose terms are sums of four squares, the same with sum_j e"""
    c = po.cfg(po.QAM64, po.C7_8, po.T8k, po.G1_4)
    iq = po.tx(c, po.make_ts(po.packets_per_superframe(c), 11), scale=1.0)
    iq = po.channel(iq, c.N, cfo=0.37, snr_db=3.0, seed=11)[CUT:CUT + 17 * 10240 + 8192 + 5]
    for h in range(scanref.HYPS):
        J, A, E = scanref.fold32(iq, h)
        J2, A2, E2, mag, en = scanref.fold64(iq, h)
        assert J == J2 > 16
        bound = 20.0 * 2.0 ** -24
        assert (np.abs(A.real - A2.real) <= bound * mag).all() and (np.abs(A.imag - A2.imag) <= bound * mag).all(), h
        assert (np.abs(E - E2) <= bound * en).all(), h
        assert np.abs(A - A2).max() > 0, "the two models are not the same arithmetic"
