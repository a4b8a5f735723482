"""The RF front-end block's specification as a numpy model (include/dvbt_hip.h, dvbt_rf_*): the transmitter's amplifier, oscillator phase noise as a sum of
tones, the tuner's IQ imbalance and DC offset, in this order, each off by default.

    1. u = x (1 + (|x|^2 / A^2)^p)^(-1/(2p))                   Rapp AM/AM; A = 0: off; p = 0 stands for 2
    2. r = u cis(phi(n))     phi(n) = sum_m a_m sin(2 pi theta_m(n))     theta_m(n) = top 32 bits of (ph_m + inc_m n mod 2^64), scaled by 2^-32
    3. v = mu r + nu conj(r)                                   mu = 0 stands for 1
    4. y = v + dc

n is the absolute sample index: first_sample + the index in the array.  The phases are integers (uint64 arrays wrap mod 2^64); everything else is float64
here and float32 on the device.  tones() turns a phase-noise mask into the tone table (dvbt_rf_phase_noise_tones is the same formulas in C).
"""
import math
from collections import namedtuple

import numpy as np

from chanref import philox4x32

MAX_TONES, MAX_MASK_POINTS = 32, 8
TAG = 0x5246504E                                   # "RFPN": counter word 3; the noise generator leaves it 0, the fading table has "FADE"
SAMPLE_RATE = 64e6 / 7

Params = namedtuple("Params", "sat_amplitude smoothness tones mu nu dc")


def params(sat_amplitude=0.0, smoothness=2.0, tones=None, mu=1, nu=0, dc=0):
    """tones: (inc, phase, amp), three sequences of equal length, or None; the floats are rounded to float32 as the C struct holds them"""
    inc, ph, amp = ((), (), ()) if tones is None else tones
    t = (tuple(int(v) for v in inc), tuple(int(v) for v in ph), tuple(float(np.float32(v)) for v in amp))
    assert len(t[0]) == len(t[1]) == len(t[2]) <= MAX_TONES
    mu = complex(np.complex64(mu))
    return Params(float(np.float32(sat_amplitude)), float(np.float32(smoothness)) or 2.0, t, mu if mu != 0 else 1.0 + 0j, complex(np.complex64(nu)),
                  complex(np.complex64(dc)))


# ------------------------------------------------------------------ the stages
def pa(x, A, p=2.0):
    """Rapp AM/AM in float64 for every finite x: above |x| = A in the form t^(-1/2) (1 + t^(-p))^(-1/(2p)), t = |x|^2 / A^2, which cannot overflow"""
    x = np.asarray(x).astype(np.complex128)
    if A == 0:
        return x
    p = float(p) or 2.0
    r = np.abs(x) / float(A)                                       # np.abs of a complex is hypot: no overflow
    g = np.ones(x.shape, np.float64)
    lo = r <= 1.0
    g[lo] = (1.0 + r[lo] ** (2.0 * p)) ** (-1.0 / (2.0 * p))
    hi = ~lo
    g[hi] = (1.0 + r[hi] ** (-2.0 * p)) ** (-1.0 / (2.0 * p)) / r[hi]
    return x * g


def phi(tones, first, count):
    """phi(n) for n = first .. first + count - 1, float64; the phases as uint64 products, which wrap mod 2^64"""
    inc, ph, amp = tones
    n = (int(first) + np.arange(count, dtype=np.uint64)).astype(np.uint64) if count else np.zeros(0, np.uint64)
    if count and int(first) + count > 2 ** 63:
        raise ValueError("sample index beyond 2^63")
    out = np.zeros(count, np.float64)
    for a, b, c in zip(inc, ph, amp):
        acc = n * np.uint64(a) + np.uint64(b)
        theta = (acc >> np.uint64(32)).astype(np.float64) * 2.0 ** -32
        out = out + c * np.sin(2.0 * np.pi * theta)
    return out


def phase_noise(x, tones, first=0):
    x = np.asarray(x).astype(np.complex128)
    if not len(tones[0]):
        return x
    return x * np.exp(1j * phi(tones, first, len(x)))


def iq(x, mu=1, nu=0):
    x = np.asarray(x).astype(np.complex128)
    return complex(mu) * x + complex(nu) * np.conj(x)


def rf(x, p, first_sample=0):
    """the model: complex128 out (the block rounds to complex64)"""
    y = pa(x, p.sat_amplitude, p.smoothness)
    y = phase_noise(y, p.tones, first_sample)
    if not (p.mu == 1 and p.nu == 0):
        y = iq(y, p.mu, p.nu)
    return y + p.dc if p.dc != 0 else y


# ------------------------------------------------------------------ the helpers of gr_dvbt_amd.RfFrontend
def saturation(ibo_db, ref_power):
    """the amplifier's saturation amplitude for an input back-off of ibo_db relative to the mean power ref_power"""
    return math.sqrt(ref_power * 10.0 ** (ibo_db / 10.0))


def iq_imbalance(gain_db, phase_deg):
    """(mu, nu) of a tuner whose Q arm has gain_db more gain and phase_deg of skew"""
    g, psi = 10.0 ** (gain_db / 20.0), math.radians(phase_deg)
    return (1.0 + g * np.exp(-1j * psi)) / 2.0, (1.0 - g * np.exp(1j * psi)) / 2.0


def irr_db(mu, nu):
    """image rejection ratio"""
    return 10.0 * math.log10(abs(mu) ** 2 / abs(nu) ** 2)


# ------------------------------------------------------------------ the tone table of a phase-noise mask
def mask_level(points, f):
    """L(f) as a power ratio per Hz: linear in dB over log f between the points"""
    fs, db = [q[0] for q in points], [q[1] for q in points]
    return 10.0 ** (np.interp(np.log(f), np.log(fs), db) / 10.0)


def mask_integral(points, lo, hi):
    """the integral of L over [lo, hi] in closed form, segment by segment: L = l_k (f / f_k)^s on segment k"""
    total = 0.0
    for (fa, da), (fb, db) in zip(points[:-1], points[1:]):
        a, b = max(lo, fa), min(hi, fb)
        if not b > a:
            continue
        s = (db - da) / (10.0 * math.log10(fb / fa))
        w = math.log(b / a)
        F = w if abs(s + 1.0) < 1e-9 else math.expm1((s + 1.0) * w) / (s + 1.0)
        total += 10.0 ** (da / 10.0) * (a / fa) ** s * a * F
    return total


def edges(points, M):
    f0, fl = float(points[0][0]), float(points[-1][0])
    lr = math.log(fl / f0)
    return [f0 if m == 0 else (fl if m == M else f0 * math.exp(lr * m / M)) for m in range(M + 1)]


def tone_freqs(points, M, seed):
    """f_m in Hz, before the rounding to an increment"""
    seed = int(seed) & 0xffffffffffffffff
    f0, fl = float(points[0][0]), float(points[-1][0])
    lr = math.log(fl / f0)
    w = philox4x32((np.arange(M), 0, 0, TAG), (seed & 0xffffffff, seed >> 32)).reshape(M, 4)
    return [f0 * math.exp(lr * (m + (float(w[m, 0]) + 0.5) * 2.0 ** -32) / M) for m in range(M)]


def tones(points, n_tones=32, seed=0, sample_rate=SAMPLE_RATE):
    """(inc, phase, amp): two lists of Python ints below 2^64 and a float32 array"""
    points = [(float(f), float(d)) for f, d in points]
    M = int(n_tones)
    seed = int(seed) & 0xffffffffffffffff
    w = philox4x32((np.arange(M), 0, 0, TAG), (seed & 0xffffffff, seed >> 32)).reshape(M, 4)
    e = edges(points, M)
    f = tone_freqs(points, M, seed)
    inc = [int(round(f[m] / sample_rate * 2.0 ** 64)) for m in range(M)]      # the scaling is exact; round() of a float is to nearest even
    ph = [(int(w[m, 1]) << 32) | int(w[m, 2]) for m in range(M)]
    amp = np.array([2.0 * math.sqrt(mask_integral(points, e[m], e[m + 1])) for m in range(M)], dtype=np.float32)
    return inc, ph, amp


def rms_deg(tones_):
    """the rms phase of a tone table in degrees: sqrt(sum a^2 / 2)"""
    return math.degrees(math.sqrt(float(np.sum(np.asarray(tones_[2], np.float64) ** 2) / 2.0)))
