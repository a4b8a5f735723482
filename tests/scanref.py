"""The signal scanner (dvbt_scan_*) in numpy: the text of include/dvbt_hip.h's "scan" block, operation by operation.

fold32    the device's sums: float32 terms, every product and sum rounded on its own, groups of SCAN_GROUP symbols added in float32 in ascending symbol order
          from +0, closed groups added to doubles in ascending order, the open group last -- the device's bits
fold64    the same sums in plain float64, with sum_j |a||b| and sum_j e per bin (what the float32 sums are bounded against)
evaluate  the host's double arithmetic (dvbt_scan_evaluate), in Python floats: the same operations in the same order
"""
import math
import numpy as np

HYPS = 8
GROUP = 16
MIN_SAMPLES = 8 * 10240 + 8192
RHO_MIN, RATIO_MIN = 0.1, 1.5


def dims(h):
    """(N, G, S) of hypothesis h = 4 mode + guard"""
    N = 8192 if h >> 2 else 2048
    G = N >> (5 - (h & 3))
    return N, G, N + G


def symbols(samples, h):
    N, _, S = dims(h)
    return (samples - N) // S if samples >= N else 0


def _terms(x, h, dtype):
    N, _, S = dims(h)
    J = symbols(len(x), h)
    a, b = x[:J * S].reshape(J, S), x[N:N + J * S].reshape(J, S)
    ar, ai, br, bi = (np.ascontiguousarray(v, dtype=dtype) for v in (a.real, a.imag, b.real, b.imag))
    re = ar * br + ai * bi
    im = ai * br - ar * bi
    en = (ar * ar + ai * ai) + (br * br + bi * bi)
    return J, S, re, im, en


def fold32(x, h):
    """(J, A complex128 [S], E float64 [S]) of the complex64 stream x for hypothesis h, as the device forms them"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    with np.errstate(all="ignore"):
        J, S, re, im, en = _terms(x, h, np.float32)
        out = [np.zeros(S, np.float64) for _ in range(3)]
        for g0 in range(0, J, GROUP):
            for t, o in zip((re, im, en), out):
                acc = np.zeros(S, np.float32)
                for j in range(g0, min(g0 + GROUP, J)):
                    acc = acc + t[j]
                o += acc.astype(np.float64)            # closed groups in ascending order, then the open one: one loop, the same order
    A = np.empty(S, np.complex128)
    A.real, A.imag = out[0], out[1]                    # (not re + 1j im: that turns an inf into a NaN)
    return J, A, out[2]


def fold64(x, h):
    """(J, A, E, sum_j |a||b|, sum_j e) per bin in float64"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    J, S, re, im, en = _terms(x, h, np.float64)
    N = dims(h)[0]
    mag = (np.abs(x[:J * S].astype(np.complex128)) * np.abs(x[N:N + J * S].astype(np.complex128))).reshape(J, S)
    return J, re.sum(axis=0) + 1j * im.sum(axis=0), en.sum(axis=0), mag.sum(axis=0), en.sum(axis=0)


def evaluate_one(h, J, A, E):
    """(rho, symbol_start, cfo) of one hypothesis"""
    if J <= 0:
        return 0.0, 0, 0.0
    _, G, S = dims(h)
    Ar, Ai, Ev = [float(v) for v in np.real(A)], [float(v) for v in np.imag(A)], [float(v) for v in E]
    sr = si = se = 0.0
    for m in range(S):
        sr = sr + Ar[m]
        si = si + Ai[m]
        se = se + Ev[m]
    if not (math.isfinite(sr) and math.isfinite(si) and math.isfinite(se)):
        return math.nan, 0, 0.0
    mr, mi = sr / S, si / S
    ar, ai = [v - mr for v in Ar], [v - mi for v in Ai]
    cr = ci = ph = 0.0
    for k in range(G):
        cr = cr + ar[k]
        ci = ci + ai[k]
        ph = ph + Ev[k]
    best, bm, bcr, bci, bph = cr * cr + ci * ci, 0, cr, ci, ph
    for m in range(S - 1):
        t = m + G if m + G < S else m + G - S
        cr = (cr - ar[m]) + ar[t]
        ci = (ci - ai[m]) + ai[t]
        ph = (ph - Ev[m]) + Ev[t]
        q = cr * cr + ci * ci
        if q > best:
            best, bm, bcr, bci, bph = q, m + 1, cr, ci, ph
    rho = math.sqrt(best) / (bph / 2.0) if bph > 0.0 else 0.0
    cfo = -math.atan2(bci, bcr) / (2.0 * math.pi)
    return rho, bm, 0.5 if cfo == -0.5 else cfo


def evaluate(J, A, E, samples, nonfinite=0, rho_min=0.0, ratio_min=0.0):
    """dvbt_scan_evaluate: J[8], A[8], E[8] -> dict(detected, mode, guard, rho, symbol_start, cfo, symbols, samples_pushed, nonfinite)"""
    rho_min, ratio_min = rho_min or RHO_MIN, ratio_min or RATIO_MIN
    one = [evaluate_one(h, J[h], A[h], E[h]) for h in range(HYPS)]
    rho = [o[0] for o in one]
    b = 0
    for h in range(1, HYPS):
        if rho[h] > rho[b]:
            b = h
    r = -1
    for h in range(HYPS):
        if h != b and (r < 0 or rho[h] > rho[r]):
            r = h
    det = (all(j >= 8 for j in J) and all(math.isfinite(v) for v in rho) and nonfinite == 0
           and rho[b] >= rho_min and rho[b] >= ratio_min * rho[r])
    return dict(detected=int(det), mode=b >> 2 if det else -1, guard=b & 3 if det else -1, rho=rho, symbol_start=[o[1] for o in one],
                cfo=[o[2] for o in one], symbols=[int(j) for j in J], samples_pushed=int(samples), nonfinite=int(nonfinite), best=b, runner_up=r)


def scan(x, fold=fold32, **kw):
    """fold and evaluate a whole stream"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    f = [fold(x, h) for h in range(HYPS)]
    bad = int(np.count_nonzero(~(np.isfinite(x.real) & np.isfinite(x.imag))))
    return evaluate([v[0] for v in f], [v[1] for v in f], [v[2] for v in f], len(x), bad, **kw)
