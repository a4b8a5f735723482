"""The spectrum analyser's specification as a numpy model in float64 (include/dvbt_hip.h, dvbt_spectrum_*).

    segment k = x[k hop : k hop + N], every complete one; S of them
    psd[b]    = sum_k |FFT(w x_k)[(b - N/2) mod N]|^2 / (S N sum w^2)          w: the float32 table of the periodic window
    statistics over x[0 : S hop]: sum |x|^2, max |x|^2, hist[float_bits(|x|^2) >> 20]++   with |x|^2 = fmaf(re, re, im im) in float32

welch() returns a Reading, whose helpers (shoulder, occupied bandwidth, CCDF, PAPR, mask margin) are what gr_dvbt_amd.SpectrumReading's must equal.
"""
import numpy as np

HIST_BINS = 2048
SAMPLE_RATE = 64e6 / 7
RECT, HANN, BH4 = 0, 1, 2
GROUP = 32


def window(N, kind):
    t = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
    if kind == RECT:
        w = np.ones(N)
    elif kind == HANN:
        w = 0.5 - 0.5 * np.cos(t)
    elif kind == BH4:
        w = 0.35875 - 0.48829 * np.cos(t) + 0.14128 * np.cos(2.0 * t) - 0.01168 * np.cos(3.0 * t)
    else:
        raise ValueError(kind)
    return w.astype(np.float32)


def enbw(N, kind):
    w = window(N, kind).astype(np.float64)
    return N * (w * w).sum() / w.sum() ** 2


def segments(n, N, hop):
    return (n - N) // hop + 1 if n >= N else 0


def power32(x):
    """fmaf(re, re, im * im) in float32, correctly rounded: re^2 is exact in a double; the sum with the rounded im^2 is rounded to odd in double, which
    then rounds to float32 as the exact sum would"""
    x = np.asarray(x, dtype=np.complex64)
    re, im = x.real.astype(np.float64), x.imag
    with np.errstate(all="ignore"):
        p, q = re * re, (im * im).astype(np.float64)                   # im * im: one float32 rounding
        s = p + q
        bb = s - p
        e = (p - (s - bb)) + (q - bb)                                  # TwoSum: s + e is the exact sum
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        bits = s.view(np.int64).copy()
        bits[fix] += np.where(e[fix] > 0, 1, -1)                       # s > 0 here: towards e, onto an odd mantissa
        return bits.view(np.float64).astype(np.float32)


def bins_of(p32):
    """histogram bin of float32 powers: the bits without the sign, >> 20"""
    return ((np.asarray(p32, dtype=np.float32).view(np.uint32) & np.uint32(0x7fffffff)) >> np.uint32(20)).astype(np.int64)


class Reading:
    def __init__(self, psd, hist, segments, samples_pushed, samples_counted, nonfinite, sum_power, peak_power, fft_size, hop, window, sample_rate=SAMPLE_RATE,
                 pmax=0.0):
        self.psd, self.hist = np.asarray(psd, dtype=np.float64), np.asarray(hist, dtype=np.uint64)
        self.segments, self.samples_pushed, self.samples_counted, self.nonfinite = segments, samples_pushed, samples_counted, nonfinite
        self.sum_power, self.peak_power = float(sum_power), np.float32(peak_power)
        self.fft_size, self.hop, self.window, self.sample_rate = fft_size, hop, window, float(sample_rate)
        self.pmax = pmax                                               # the largest bin of a single segment, |X|^2 / (N sum w^2)

    def freqs(self, sample_rate=None):
        fs = self.sample_rate if sample_rate is None else float(sample_rate)
        return (np.arange(self.fft_size) - self.fft_size // 2) * (fs / self.fft_size)

    @property
    def mean_power(self):
        return self.sum_power / self.samples_counted if self.samples_counted else 0.0

    @property
    def enbw(self):
        return enbw(self.fft_size, self.window)

    def band_power(self, f_lo, f_hi):
        f = self.freqs()
        return float(self.psd[(f >= f_lo) & (f <= f_hi)].sum())

    def occupied_bandwidth(self, fraction=0.99):
        c, total = self.fft_size // 2, float(self.psd.sum())
        m = 0
        while m < c and float(self.psd[max(c - m, 0):c + m + 1].sum()) < fraction * total:
            m += 1
        if float(self.psd[max(c - m, 0):c + m + 1].sum()) < fraction * total:
            return self.sample_rate
        return (2 * m + 1) * self.sample_rate / self.fft_size

    def inband(self, half_bandwidth):
        return float(self.psd[np.abs(self.freqs()) <= 0.9 * half_bandwidth].mean())

    def shoulder_db(self, half_bandwidth, lo=300e3, hi=700e3):
        if half_bandwidth + hi > self.sample_rate / 2:
            raise ValueError("beyond Nyquist")
        f, ref = self.freqs(), self.inband(half_bandwidth)
        out = []
        for side in (-1.0, 1.0):
            d = side * f - half_bandwidth
            out.append(10.0 * np.log10(ref / float(self.psd[(d >= lo) & (d <= hi)].max())))
        return tuple(out)

    def ccdf(self):
        j = np.arange(1, 2040, dtype=np.uint32)
        edges = (j << np.uint32(20)).view(np.float32).astype(np.float64)
        h = self.hist.astype(np.float64)
        above = np.array([h[k:].sum() for k in j])
        return 10.0 * np.log10(edges / self.mean_power), above / float(self.samples_counted)

    def papr_db(self, prob=None):
        if prob is None:
            return 10.0 * np.log10(float(self.peak_power) / self.mean_power)
        lev, p = self.ccdf()
        j = next(k for k in range(len(p)) if p[k] <= prob)
        if j == 0:
            return float(lev[0])
        return float(lev[j - 1] + (lev[j] - lev[j - 1]) * (p[j - 1] - prob) / (p[j - 1] - p[j]))

    def mask_margin(self, points, half_bandwidth):
        pts = sorted((float(o), float(d)) for o, d in points)
        off, db = [o for o, _ in pts], [d for _, d in pts]
        if len(pts) < 2 or off[0] < 0 or off[-1] > self.sample_rate / 2:
            raise ValueError("bad mask")
        f, ref = np.abs(self.freqs()), self.inband(half_bandwidth)
        worst = np.inf
        for b in range(self.fft_size):
            if off[0] <= f[b] <= off[-1]:
                with np.errstate(divide="ignore"):
                    worst = min(worst, float(np.interp(f[b], off, db)) - 10.0 * np.log10(self.psd[b] / ref))
        return float(worst)


def welch(x, N, hop=0, kind=HANN, sample_rate=SAMPLE_RATE):
    """the model of one handle that was pushed all of x"""
    x = np.asarray(x, dtype=np.complex64)
    hop = hop or N // 2
    assert N >= 64 and N <= 8192 and N & (N - 1) == 0 and N // 8 <= hop <= N and kind in (RECT, HANN, BH4)
    S = segments(len(x), N, hop)
    w = window(N, kind).astype(np.float64)
    acc, pmax = np.zeros(N), 0.0
    x128 = x.astype(np.complex128)
    with np.errstate(all="ignore"):
        for k0 in range(0, S, 256):                                    # 256 segments at a time
            idx = (np.arange(k0, min(S, k0 + 256)) * hop)[:, None] + np.arange(N)[None, :]
            P = np.abs(np.fft.fftshift(np.fft.fft(x128[idx] * w[None, :], axis=1), axes=1)) ** 2
            acc += P.sum(axis=0)
            pmax = max(pmax, float(P.max()) if np.isfinite(P).all() else float(np.nanmax(np.where(np.isfinite(P), P, 0.0))))
    norm = S * N * float((w * w).sum())
    psd = acc / norm if S else np.zeros(N)
    counted = x[:S * hop]
    p32 = power32(counted)
    hist = np.bincount(bins_of(p32), minlength=HIST_BINS).astype(np.uint64)
    with np.errstate(all="ignore"):
        sum_power = float(p32.astype(np.float64).sum())
    bits = p32.view(np.uint32) & np.uint32(0x7fffffff)
    peak = np.array([bits.max() if len(bits) else 0], dtype=np.uint32).view(np.float32)[0]
    return Reading(psd, hist, S, len(x), S * hop, int(hist[2040:].sum()), sum_power, peak, N, hop, kind, sample_rate, pmax / (N * float((w * w).sum())))
