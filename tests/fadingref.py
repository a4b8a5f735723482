"""The fading block's specification as a numpy model (include/dvbt_hip.h, dvbt_fading_*): a tapped delay line whose taps fade as sums of sinusoids.

    y[n] = sum_{i < n_paths} g_i(n) x[n - d_i]          x[k] = 0 in front of the stream's first sample; i ascending, the first product starts the sum

n is the absolute sample index: first_sample + the index in the array.  The sinusoid table (inc, ph) is integers, computed in double by operations that
give the same bits everywhere (dvbt_fading_table is equal to table() word for word); everything behind it is float64 here and float32 on the device.

    table     w = philox4x32_10((m, i, 0, TAG), (seed lo, seed hi));  u = (w0 + 0.5) 2^-32;  alpha = (m + u) / M turns;  f = doppler cos(2 pi alpha)
              inc[i][m] = nearbyint(f 2^64) mod 2^64;  ph[i][m] = (w1 << 32) | w2
    knots     every KNOT = 64 absolute samples: S_i(k) = sum_m cis(top 32 bits of (ph + inc 64 k mod 2^64)),  G_i(k) = los_i + s_i S_i(k),
              s_i = float32(sigma_i / sqrt(M))
    gain      k = n >> 6, t = (n & 63) / 64:  g_i(n) = G_i(k) + t (G_i(k + 1) - G_i(k))

The piecewise-linear gain is the specification; exact_gains() is the sum it interpolates, at most chord_bound() away.
"""
import math
from collections import namedtuple

import numpy as np

from chanref import philox4x32

MAX_PATHS, MAX_DELAY, MAX_SINUSOIDS, KNOT = 24, 8192, 32, 64
TAG = 0x46414445                                   # "FADE": counter word 3, which the noise generator leaves 0
MAX_DOPPLER = 2.0 ** -12
TWO_PI = 6.283185307179586

Params = namedtuple("Params", "paths doppler n_sinusoids seed")


def params(paths, doppler=0.0, n_sinusoids=16, seed=0):
    """paths: ((delay, los, sigma), ...); los and sigma are rounded to float32 as the C struct holds them; n_sinusoids 0 is 16"""
    ps = tuple((int(d), complex(np.complex64(los)), float(np.float32(s))) for d, los, s in paths)
    return Params(ps, float(doppler), int(n_sinusoids) or 16, int(seed) & 0xffffffffffffffff)


def cos_turns(alpha):
    """cos(2 pi alpha) for alpha in [0, 1] from IEEE double + - * / alone, in this order (dvbt_fading.inc::fading_cos_turns is the same line by line):
    the nearest quarter turn comes off, the rest (|x| <= pi / 4) goes through the Taylor series of cos and sin, 12 terms behind the first."""
    q = int(math.floor(alpha * 4.0 + 0.5))
    x = (alpha - q * 0.25) * TWO_PI
    z = x * x
    c, s, ct, st = 1.0, x, 1.0, x
    for k in range(1, 13):
        ct = -ct * z / float((2 * k - 1) * (2 * k))
        c = c + ct
        st = -st * z / float((2 * k) * (2 * k + 1))
        s = s + st
    return (c, -s, -c, s)[q & 3]


def table(p):
    """(inc, ph): two lists [n_paths][M] of Python ints below 2^64"""
    M = p.n_sinusoids
    inc, ph = [], []
    for i in range(len(p.paths)):
        w = philox4x32((np.arange(M), i, 0, TAG), (p.seed & 0xffffffff, p.seed >> 32)).reshape(M, 4)
        ri, rp = [], []
        for m in range(M):
            u = (float(w[m, 0]) + 0.5) * 2.0 ** -32
            alpha = (float(m) + u) / float(M)
            f = p.doppler * cos_turns(alpha)
            ri.append(int(round(f * 2.0 ** 64)) % 2 ** 64)          # f 2^64 is exact and below 2^53: round() is nearbyint (ties to even)
            rp.append((int(w[m, 1]) << 32) | int(w[m, 2]))
        inc.append(ri)
        ph.append(rp)
    return inc, ph


def freqs(p):
    """the sinusoids' frequencies in cycles per sample, float64 [n_paths][M], from the integer table"""
    inc, _ = table(p)
    a = np.array(inc, dtype=object)
    return np.array([[(v - 2 ** 64 if v >= 2 ** 63 else v) / 2.0 ** 64 for v in row] for row in a], dtype=np.float64)


def _cis_sum(inc_row, ph_row, ns):
    """sum_m exp(2 pi j top32(ph + inc n mod 2^64) / 2^32) for the absolute indices ns (Python ints), m ascending"""
    S = np.zeros(len(ns), np.complex128)
    nn = np.array(ns, dtype=np.uint64).reshape(-1)
    for a, b in zip(inc_row, ph_row):
        acc = nn * np.uint64(a) + np.uint64(b)                     # uint64 arrays wrap mod 2^64
        top = (acc >> np.uint64(32)).astype(np.float64) * 2.0 ** -32
        S = S + np.exp(2j * np.pi * top)
    return S


def _scale(p, i):
    return float(np.float32(p.paths[i][2] / math.sqrt(float(p.n_sinusoids))))


def knots(p, k0, count):
    """G_i(k) for k = k0 .. k0 + count - 1: complex128 [n_paths][count]"""
    inc, ph = table(p)
    ns = [KNOT * (int(k0) + k) for k in range(count)]
    return np.stack([p.paths[i][1] + _scale(p, i) * _cis_sum(inc[i], ph[i], ns) for i in range(len(p.paths))])


def gains(p, first, count):
    """g_i(n) for n = first .. first + count - 1: complex128 [n_paths][count]"""
    first = int(first)
    k0 = first >> 6
    nk = ((first + max(count, 1) - 1) >> 6) - k0 + 2
    G = knots(p, k0, nk)
    n = first + np.arange(count, dtype=np.int64)
    k = (n >> 6) - k0
    t = (n & 63).astype(np.float64) / 64.0
    return G[:, k] + t * (G[:, k + 1] - G[:, k])


def exact_gains(p, first, count):
    """the sum of sinusoids at every sample, not interpolated: complex128 [n_paths][count]"""
    inc, ph = table(p)
    ns = [int(first) + j for j in range(count)]
    return np.stack([p.paths[i][1] + _scale(p, i) * _cis_sum(inc[i], ph[i], ns) for i in range(len(p.paths))])


def chord_bound(p, i):
    """largest distance of path i's gain from exact_gains: M chords of unit phasors that turn by at most 2 pi 64 doppler between two knots"""
    return p.paths[i][2] * math.sqrt(float(p.n_sinusoids)) * (2.0 * math.pi * KNOT * p.doppler) ** 2 / 8.0


def fading(x, p, first_sample=0):
    """the model: complex128 out (the block rounds to complex64)"""
    x = np.asarray(x).astype(np.complex128)
    first, count = int(first_sample), len(x)
    y = np.zeros(count, np.complex128)
    if count == 0:
        return y
    k0 = first >> 6
    G = knots(p, k0, ((first + count - 1) >> 6) - k0 + 2)
    n = first + np.arange(count, dtype=np.int64)
    k = (n >> 6) - k0
    t = (n & 63).astype(np.float64) / 64.0
    for i, (d, _, _) in enumerate(p.paths):                      # one path's gains at a time: a long stream times 24 paths need not exist at once
        if d < count:
            g = G[i, k[d:]] + t[d:] * (G[i, k[d:] + 1] - G[i, k[d:]])
            y[d:] += g * x[:count - d]
    return y


TU6_DELAYS_US = (0.0, 0.2, 0.5, 1.6, 2.3, 5.0)
TU6_POWERS_DB = (-3.0, 0.0, -2.0, -6.0, -8.0, -10.0)


def tu6(doppler_hz, sample_rate=64e6 / 7, rice_k_db=None):
    """COST 207 TU6 as (paths, doppler in cycles per sample): delays rounded to samples, powers normalised to a total of 1; with rice_k_db the scatter is
    scaled by 1 / (1 + K) in power and a fixed part sqrt(K / (1 + K)) stands on path 0"""
    pw = [10.0 ** (d / 10.0) for d in TU6_POWERS_DB]
    tot = sum(pw)
    K = None if rice_k_db is None else 10.0 ** (rice_k_db / 10.0)
    scat = 1.0 if K is None else 1.0 / (1.0 + K)
    paths = []
    for i, (us, w) in enumerate(zip(TU6_DELAYS_US, pw)):
        los = math.sqrt(K / (1.0 + K)) if (K is not None and i == 0) else 0.0
        paths.append((int(round(us * 1e-6 * sample_rate)), complex(los), math.sqrt(w / tot * scat)))
    return tuple(paths), float(doppler_hz) / float(sample_rate)
