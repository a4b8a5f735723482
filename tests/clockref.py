"""The sample-clock offset block's specification as a numpy model (include/dvbt_hip.h, dvbt_clock_*): positions as Python ints, everything else in float64.

    S = 2^64 + rint(ppm 1e-6 2^64)   P0 = trunc(start 2^64)   P(m) = P0 + m S   base = P >> 64   f = P mod 2^64   H = taps / 2
    y[m] = sum_{k = -(H-1)}^{H} h(k - f / 2^64) x[base + k]      h(a) = sinc(a) (0.54 + 0.46 cos(pi a / (H + 1)))      x[i] = 0 for i < first_in
    f == 0: y[m] = x[base]

m and the x index are absolute: the array handed to resample() begins at x[first_in], what it returns at y[max(E(first_in), first_out)].
E(N) = the smallest m >= 0 with base(m) + H >= N: N inputs complete the outputs in front of it.
"""
from fractions import Fraction

import numpy as np

TWO64 = 1 << 64


def step(ppm):
    """S: ppm 1e-6 is one double product, the scaling is exact, the rounding is to nearest even"""
    return TWO64 + int(np.rint(np.ldexp(np.float64(ppm) * np.float64(1e-6), 64)))


def p0(start):
    return int(Fraction(float(start)) * TWO64)          # int() truncates; start >= 0


def pos(m, ppm, start):
    """(base, f) of output m"""
    return divmod(p0(start) + int(m) * step(ppm), TWO64)


def E(N, ppm, start, taps=16):
    """the smallest m >= 0 with base(m) + H >= N"""
    need = (int(N) - taps // 2) * TWO64 - p0(start)       # P(m) >= (N - H) 2^64
    return max(0, -((-need) // step(ppm)))


def next_output(n_in_total, ppm, start, taps=16, first_out=0, first_in=0):
    return max(E(first_in + n_in_total, ppm, start, taps), first_out)


def outputs(n_in_total, ppm, start, taps=16, first_out=0, first_in=0):
    """outputs emitted once n_in_total inputs have been pushed"""
    return next_output(n_in_total, ppm, start, taps, first_out, first_in) - next_output(0, ppm, start, taps, first_out, first_in)


def first_in_for(first_out, ppm, start, taps=16):
    """the first input a piece that begins at output first_out needs: base(first_out) - (H - 1)"""
    return pos(first_out, ppm, start)[0] - (taps // 2 - 1)


def h(a, taps):
    return np.sinc(a) * (0.54 + 0.46 * np.cos(np.pi * a / (taps // 2 + 1)))


def resample(x, ppm, start=None, taps=16, first_out=0, first_in=0):
    """the model: every output that x = (x[first_in], x[first_in + 1], ...) completes, complex128 (the block rounds to complex64)"""
    H = taps // 2
    start = float(H if start is None else start)
    x = np.asarray(x).astype(np.complex128)
    m0 = next_output(0, ppm, start, taps, first_out, first_in)
    m1 = next_output(len(x), ppm, start, taps, first_out, first_in)
    out = np.zeros(m1 - m0, np.complex128)
    if m1 == m0:
        return out
    P0, S = p0(start), step(ppm)
    xp = np.concatenate([np.zeros(taps, np.complex128), x])          # xp[i + taps] = x[first_in + i]: a tap in front of the array reads a zero
    org = first_in - taps
    k = np.arange(-(H - 1), H + 1)
    chunk = 1 << 15
    for a in range(m0, m1, chunk):
        b = min(m1, a + chunk)
        P = [P0 + m * S for m in range(a, b)]
        base = np.array([p >> 64 for p in P], dtype=object)
        f = np.array([p & (TWO64 - 1) for p in P], dtype=np.uint64)
        rel = np.array([int(v) - org for v in base], dtype=np.int64)    # index of x[base] in xp
        idx = rel[:, None] + k[None, :]                                 # m >= E(first_in): none in front of xp; m < E(first_in + len(x)): none behind it
        assert idx.min() >= 0 and idx.max() < len(xp)
        v = xp[idx]
        phi = f.astype(np.float64) * 2.0 ** -64
        # above 1/2 the argument is taken from 2^64 - f, so that the tap at k = 1 keeps its precision in float64 as well
        g = (~f + np.uint64(1)).astype(np.float64) * 2.0 ** -64
        arg = np.where((phi < 0.5)[:, None], k[None, :] - phi[:, None], (k[None, :] - 1) + g[:, None])
        y = (h(arg, taps) * v).sum(axis=1)
        whole = f == 0
        y[whole] = xp[rel[whole]]
        out[a - m0:b - m0] = y
    return out
