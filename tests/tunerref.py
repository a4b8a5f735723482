"""The tuner block (include/dvbt_hip.h, dvbt_tuner_*) in numpy: the specification, literally.

  convert   swap, then one rounded float32 multiply per component (uint8: minus 127.5 first, exact)
  mix       inc = nearbyint(shift 2^64) mod 2^64, ph(n) = n inc mod 2^64, the angle is the top 32 bits of ph; skipped where inc == 0
  resample  y[m] = sum_{k = nt-1 .. 0} br[b][k] z[n(m) - k], n(m) = floor(m M / L), b = m M mod L: the first product starts the sum, every product and
            every sum is one float32 operation

Without a shift `tuner` gives the device's bits.  With one, the device's cosine and sine are a float polynomial and the model's are numpy's, so the two
agree to rounding, not in every bit; `tuner(..., exact=True)` is the same chain in complex128 on the float32 taps (the yardstick of the tolerance tests).
`design` mirrors dvbt_tuner_design in double."""
import math
from fractions import Fraction

import numpy as np

CF32, CS16, CS8, CU8 = range(4)
DTYPES = (np.dtype(np.complex64), np.dtype(np.int16), np.dtype(np.int8), np.dtype(np.uint8))
BYTES = (8, 4, 2, 2)
SCALES = (1.0, 1.0 / 32768, 1.0 / 128, 1.0 / 127.5)
PASS_EDGE, STOP_EDGE, ATTEN_DB = 0.42, 0.58, 70.0
MAX_L, MAX_M, MAX_RATIO, MAX_NT, MAX_BRANCH_FLOATS = 128, 1024, 8, 320, 8192


def reduce(L, M):
    g = math.gcd(L, M)
    return L // g, M // g


def izero(x):
    """Io by its power series, the loop of dvbt_tables.hpp::resampler_taps, on an array"""
    x = np.asarray(x, np.float64)
    s, u, half = np.ones_like(x), np.ones_like(x), x / 2.0
    n = 1
    while True:
        t = half / n
        n += 1
        u = u * (t * t)
        s = s + u
        if (u < 1e-21 * s).all():
            return s


def design(L, M, pass_edge=PASS_EDGE, stop_edge=STOP_EDGE, atten_db=ATTEN_DB):
    """the designed prototype as float32 (the rule of the header, in double)"""
    L, M = reduce(L, M)
    A, stop = float(atten_db), float(stop_edge)
    if L > M:
        stop = min(stop, M / L - pass_edge)
    if not stop > pass_edge:
        raise ValueError("no room between the pass band and the first image")
    fp, fs = pass_edge / M, stop / M
    fc = (fp + fs) / 2.0
    beta = 0.1102 * (A - 8.7) if A > 50.0 else 0.5842 * (A - 21.0) ** 0.4 + 0.07886 * (A - 21.0)
    ntaps = int(math.ceil((A - 7.95) / (2.285 * 2.0 * math.pi * (fs - fp)))) + 1
    ntaps += 1 - (ntaps & 1)
    nt = -(-ntaps // L)
    if nt > MAX_NT or L * nt > MAX_BRANCH_FLOATS:
        raise ValueError("the prototype is too long")
    c = (ntaps - 1) / 2.0
    d = np.arange(ntaps, dtype=np.float64) - c
    x = 2.0 * fc * d
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(d == 0.0, 1.0, np.sin(math.pi * x) / (math.pi * x))
    t = d / c
    h = 2.0 * fc * sinc * izero(beta * np.sqrt(np.maximum(0.0, 1.0 - t * t))) * (1.0 / float(izero(beta)))
    return (h * (L / h.sum())).astype(np.float32)


def response_db(taps, freqs, L):
    """|H| in dB relative to the DC gain L, float64, at `freqs` in cycles per sample of the prototype's rate"""
    h = np.asarray(taps, np.float64)
    i = np.arange(len(h), dtype=np.float64)
    out = np.empty(len(freqs))
    for lo in range(0, len(freqs), 512):
        f = np.asarray(freqs[lo:lo + 512], np.float64)
        out[lo:lo + 512] = np.abs(np.exp(-2j * math.pi * np.outer(f, i)) @ h)
    return 20.0 * np.log10(np.maximum(out, 1e-300) / L)


def branches(taps, L):
    """br[b][k] = h[b + k L], zero padded: (L, nt) float32"""
    taps = np.asarray(taps, np.float32)
    nt = -(-len(taps) // L)
    flat = np.zeros(L * nt, np.float32)
    flat[:len(taps)] = taps
    return flat.reshape(nt, L).T.copy()


def total(N, L, M):
    """outputs in front of the stream's input N: ceil(N L / M)"""
    return -(-(N * L) // M)


def outputs(n_in_total, L, M, first_in=0):
    L, M = reduce(L, M)
    return total(first_in + n_in_total, L, M) - total(first_in, L, M)


def first_whole_output(n0, ntaps, L, M):
    """from this output on a handle created with first_in = n0 equals the handle that began at 0"""
    L, M = reduce(L, M)
    return total(n0 + -(-ntaps // L) - 1, L, M)


def increment(shift):
    """nearbyint(shift 2^64) mod 2^64, ties to even: exact in integers (a double is a fraction)"""
    return round(Fraction(float(shift)) * 2 ** 64) % 2 ** 64


def components(raw, fmt):
    """(I, Q) as the raw dtype's values in float32 (float for CF32), from flat interleaved or (n, 2) or complex64"""
    raw = np.asarray(raw)
    assert raw.dtype == DTYPES[fmt], (raw.dtype, fmt)
    if fmt == CF32:
        v = np.ascontiguousarray(raw).reshape(-1).view(np.float32)
    else:
        v = np.ascontiguousarray(raw).reshape(-1)
    return v[0::2].astype(np.float32), v[1::2].astype(np.float32)


def convert(raw, fmt, scale=None, swap_iq=False):
    """stage 1: complex64"""
    i, q = components(raw, fmt)
    if swap_iq:
        i, q = q, i
    s = np.float32(SCALES[fmt] if scale is None else scale)
    out = np.empty(len(i), np.complex64)
    for dst, c in ((out.real, i), (out.imag, q)):
        if fmt == CU8:
            c = c - np.float32(127.5)
        dst[...] = c if (fmt == CF32 and s == np.float32(1.0)) else c * s
    return out


def angles(n_first, count, inc):
    """2 pi (top 32 bits of ph(n)) / 2^32 for n = n_first .. n_first + count - 1, float64"""
    n = (np.arange(count, dtype=np.uint64) + np.uint64(n_first % 2 ** 64))
    with np.errstate(over="ignore"):
        ph = n * np.uint64(inc)
    return (ph >> np.uint64(32)).astype(np.float64) * (2.0 * math.pi / 2.0 ** 32)


def mix(v, inc, n_first, exact=False):
    """stage 2: float32 products and sums on float32 cosines and sines, or complex128"""
    if inc == 0:
        return v.astype(np.complex128) if exact else v
    a = angles(n_first, len(v), inc)
    if exact:
        return v.astype(np.complex128) * np.exp(1j * a)
    c, s = np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)
    out = np.empty(len(v), np.complex64)
    out.real = v.real * c - v.imag * s
    out.imag = v.real * s + v.imag * c
    return out


def resample(z, taps, L, M, first_in=0, exact=False):
    """stage 3 on a stream whose sample z[0] is input first_in: every output m with ceil(first_in L / M) <= m < ceil((first_in + len(z)) L / M)"""
    L, M = reduce(L, M)
    br = branches(taps, L)
    nt = br.shape[1]
    ft = np.float64 if exact else np.float32
    m = np.arange(total(first_in, L, M), total(first_in + len(z), L, M), dtype=np.int64)
    if len(m) == 0:
        return np.zeros(0, np.complex128 if exact else np.complex64)
    pr = m * M
    n, b = pr // L, pr % L
    pad = np.zeros(nt - 1, ft)
    zr, zi = np.concatenate([pad, z.real.astype(ft)]), np.concatenate([pad, z.imag.astype(ft)])
    base = n - first_in                        # index into the padded arrays of z[n - (nt - 1)]
    brf = br.astype(ft)
    yr = yi = None
    for i in range(nt):                        # ascending input order: tap k = nt - 1 - i
        h = brf[b, nt - 1 - i]
        pr_, pi_ = h * zr[base + i], h * zi[base + i]
        yr, yi = (pr_, pi_) if i == 0 else (yr + pr_, yi + pi_)
    out = np.empty(len(m), np.complex128 if exact else np.complex64)
    out.real, out.imag = yr, yi
    return out


def tuner(raw, fmt, L, M, shift=0.0, scale=None, taps=None, pass_edge=PASS_EDGE, stop_edge=STOP_EDGE, atten_db=ATTEN_DB, swap_iq=False, first_in=0,
          exact=False):
    """the whole block on one stream"""
    L, M = reduce(L, M)
    if taps is None:
        taps = design(L, M, pass_edge, stop_edge, atten_db)
    v = convert(raw, fmt, scale, swap_iq)
    z = mix(v, increment(shift), first_in, exact)
    return resample(z, taps, L, M, first_in, exact)


def capture_cs16(up, shift):
    """what an SDR would have recorded of the baseband `up` (already at the capture's rate): moved by `shift` cycles per sample in complex128 and quantised to
    interleaved int16 with the largest component at half of full scale"""
    x = up.astype(np.complex128) * np.exp(2j * math.pi * shift * np.arange(len(up), dtype=np.float64))
    peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    q = np.empty(2 * len(x), np.int16)
    q[0::2] = np.rint(x.real * (16384.0 / peak))
    q[1::2] = np.rint(x.imag * (16384.0 / peak))
    return q


def ts_common_packets(ts, ref):
    """ts continues ref from the position of ts's first packet in ref on: the number of packets both hold from there, all equal; 0 if the first packet
    is not found or a later one differs"""
    ts, ref = np.asarray(ts, np.uint8), np.asarray(ref, np.uint8)
    if len(ts) < 188 or len(ts) % 188 or len(ref) % 188:
        return 0
    rows = ref.reshape(-1, 188)
    at = np.flatnonzero((rows == ts[:188]).all(axis=1))
    if len(at) == 0:
        return 0
    n = min(len(ts) // 188, len(rows) - int(at[0]))
    return n if (ts[:188 * n] == ref[188 * int(at[0]):188 * (int(at[0]) + n)]).all() else 0


class Stream:
    """the model as a stream of calls: keeps the last nt - 1 values of z, as the handle does"""

    def __init__(self, fmt, L, M, shift=0.0, scale=None, taps=None, swap_iq=False, first_in=0):
        self.fmt, (self.L, self.M) = fmt, reduce(L, M)
        self.taps = design(self.L, self.M) if taps is None else np.asarray(taps, np.float32)
        self.nt = -(-len(self.taps) // self.L)
        self.inc, self.scale, self.swap = increment(shift), scale, swap_iq
        self.pos = first_in
        self.hist = np.zeros(self.nt - 1, np.complex64)

    def run(self, raw):
        z = mix(convert(raw, self.fmt, self.scale, self.swap), self.inc, self.pos)
        buf = np.concatenate([self.hist, z])
        first = self.pos - len(self.hist)
        y = resample(buf, self.taps, self.L, self.M, first)
        y = y[total(self.pos, self.L, self.M) - total(first, self.L, self.M):]
        self.pos += len(z)
        self.hist = buf[len(buf) - (self.nt - 1):] if self.nt > 1 else buf[:0]
        return y
