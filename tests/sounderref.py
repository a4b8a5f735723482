"""The channel sounder's specification (include/dvbt_hip.h, dvbt_sounder_*) as float64 numpy: the model that tests/test_sounder_model.py checks against known
channels and that tests/test_gpu_sounder_block.py holds the kernels to.  No GPU, no library: the tables are built here from the standard.

sound(rows, index, offset, cp_start, mode, window) -> Reading with `pdp` (M sums of |h|^2), `resp` (Kp sums of |E|^2) and the counts; Reading's helpers are
the ones of gr_dvbt_amd.SounderReading, line for line."""
import numpy as np

RECT, HANN = 0, 1
RUN = 8                                            # groups per slab on the device (k_sounder.hpp SND_RUN)
MAX_DELTA = 64

_CPILOT_2K = (0, 48, 54, 87, 141, 156, 192, 201, 255, 279, 282, 333, 432, 450, 483, 525, 531, 618, 636, 714, 759, 765, 780, 804, 873, 888, 918, 939, 942,
              969, 984, 1050, 1101, 1107, 1110, 1137, 1140, 1146, 1206, 1269, 1323, 1377, 1491, 1683, 1704)


class Mode:
    def __init__(self, mode):
        assert mode in (0, 1)
        self.mode = mode
        self.N, self.K = (8192, 6817) if mode else (2048, 1705)
        self.zl = -((self.K - self.N) // 2)        # ceil((N - K) / 2)
        self.Kp, self.M, self.c0 = (self.K - 1) // 3 + 1, self.N // 2, (self.K - 1) // 2
        self.cpilot = np.array(_CPILOT_2K if not mode else [k + 1704 * r for r in range(4) for k in _CPILOT_2K[:44]] + [6816])
        # w_k = 4/3 * 2 (1/2 - w_k), the PRBS X^11 + X^2 + 1 started from all ones
        w, reg = np.zeros(self.K), (1 << 11) - 1
        for k in range(self.K):
            w[k] = 4.0 * 2.0 * (0.5 - (reg & 1)) / 3.0
            reg = (reg >> 1) | ((((reg >> 2) ^ reg) & 1) << 10)
        self.w = w


def window_table(Kp, window):
    """the float32 table of window 0 (rectangular) or 1 (periodic Hann over the Kp entries), computed in double"""
    if window == RECT:
        return np.ones(Kp, np.float32)
    assert window == HANN
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(Kp, dtype=np.float64) / Kp)).astype(np.float32)


def pilot_rows(md, indices, H=None, rng=None, offset=0):
    """rows [len(indices)][N] complex128 as a modulator leaves them: scattered and continual pilots at +-4/3, unit-power QAM16 on every other carrier (none
    with rng None), times the channel H[k] (K values), moved by `offset` carriers"""
    rows = np.zeros((len(indices), md.N), np.complex128)
    k = np.arange(md.K)
    for r, x in enumerate(indices):
        v = np.zeros(md.K, np.complex128)
        if rng is not None:
            v = ((rng.randint(0, 4, md.K) * 2 - 3) + 1j * (rng.randint(0, 4, md.K) * 2 - 3)) / np.sqrt(10.0)
        pil = np.zeros(md.K, bool)
        pil[3 * (x % 4)::12] = True
        pil[md.cpilot] = True
        v[pil] = md.w[pil]
        if H is not None:
            v = v * H
        rows[r, md.zl + offset + k] = v
    return rows


def channel_of_paths(md, paths):
    """H[k] of [(delay in samples, complex amplitude)]: carrier k - c0 sits at frequency (k - c0) / N cycles per sample"""
    f = (np.arange(md.K) - md.c0) / md.N
    return sum(a * np.exp(-2j * np.pi * f * d) for d, a in paths)


def group_used(x, o, c):
    """the four indices, offsets and cp_starts of one group"""
    x, o, c = [int(v) for v in x], [int(v) for v in o], [int(v) for v in c]
    if not (0 <= x[0] <= 67 and -8 <= o[0] <= 7):
        return False
    return all(x[i] == (x[0] + i) % 68 and o[i] == o[0] and abs(c[i] - c[0]) <= MAX_DELTA for i in range(1, 4))


def sound(rows, index=None, offset=None, cp_start=None, mode=0, window=HANN, first_index=0, timing=True, phase=True, per_group=False):
    """the specification, literally.  timing=False: tau = 1; phase=False: r_i = 1 (what each correction is needed for).  per_group: also the list of
    (group, |h|^2) of the used groups."""
    md = Mode(mode)
    rows = np.asarray(rows)
    n = len(rows)
    assert rows.shape == (n, md.N)
    idx = (first_index + np.arange(n)) % 68 if index is None else np.asarray(index, np.int64)
    off = np.zeros(n, np.int64) if offset is None else np.asarray(offset, np.int64)
    cps = np.zeros(n, np.int64) if cp_start is None else np.asarray(cp_start, np.int64)
    assert len(idx) == len(off) == len(cps) == n
    win = window_table(md.Kp, window).astype(np.float64)
    pdp, resp, used, each = np.zeros(md.M), np.zeros(md.Kp), 0, []
    for g in range(n // 4):
        s = slice(4 * g, 4 * g + 4)
        if not group_used(idx[s], off[s], cps[s]):
            continue
        used += 1
        E = np.zeros(md.Kp, np.complex128)
        c_first = None
        for i in range(4):
            Y = rows[4 * g + i].astype(np.complex128)
            l, o, delta = int(idx[4 * g + i]) % 4, int(off[4 * g + i]), int(cps[4 * g + i] - cps[4 * g])

            def tau(k):
                return np.exp(-2j * np.pi * (((k - md.c0) * delta) % md.N) / md.N) if timing else np.ones(len(k))
            kc = md.cpilot
            c_i = (Y[md.zl + kc + o] * md.w[kc] * tau(kc)).sum()
            if i == 0:
                c_first = c_i
            r = c_first * np.conj(c_i)
            r = r / abs(r) if phase and np.isfinite(r) and abs(r) > 0 else 1.0
            k = np.arange(3 * l, md.K, 12)
            E[k // 3] = Y[md.zl + k + o] * md.w[k] * (9.0 / 16.0) * tau(k) * r
        x = np.zeros(md.M, np.complex128)
        x[:md.Kp] = E * win
        h = np.fft.ifft(x) * md.M / win.sum()
        p = np.abs(h) ** 2
        pdp += p
        resp += np.abs(E) ** 2
        if per_group:
            each.append((g, p))
    out = Reading(pdp, resp, n, used, n // 4 - used, mode)
    return (out, each) if per_group else out


class Reading:
    """pdp, resp and the counts, with the helpers of gr_dvbt_amd.SounderReading"""

    def __init__(self, pdp, resp, symbols_pushed, groups_used, groups_skipped, mode, sample_rate=64e6 / 7):
        self.pdp, self.resp = np.asarray(pdp, np.float64), np.asarray(resp, np.float64)
        self.symbols_pushed, self.groups_used, self.groups_skipped = int(symbols_pushed), int(groups_used), int(groups_skipped)
        self.mode, self.sample_rate = int(mode), float(sample_rate)
        self.M, self.Kp = len(self.pdp), len(self.resp)

    def delays(self, sample_rate=None):
        """the delay of every bin relative to the strongest, signed (bins from M / 2 on behind it read as pre-echoes), in samples, or in seconds for a
        sample rate"""
        m0 = int(np.argmax(self.pdp))
        d = ((np.arange(self.M) - m0 + self.M // 2) % self.M - self.M // 2) * (2.0 / 3.0)
        return d if sample_rate is None else d / float(sample_rate)

    def _five(self, m):
        return float(self.pdp[(m + np.arange(-2, 3)) % self.M].sum())

    def paths(self, threshold_db=-30.0):
        """[(delay in samples, level in dB relative to the strongest)] of the local maxima at or above the threshold, the strongest (0, 0) first, then by
        delay.  A level is the sum of the five bins around the maximum over the same sum around the strongest.  A local maximum is a bin above every other
        within five bins (3.3 samples) of it: the Hann window's main lobe is 7.2 bins wide and its first side lobe stands 4.5 bins from the centre, where the
        five bins would reach back into the main lobe."""
        p, d = self.pdp, self.delays()
        m0 = int(np.argmax(p))
        ref = self._five(m0)
        if not ref > 0.0:
            return []
        out = []
        around = np.max([np.roll(p, k) for k in range(-5, 6) if k], axis=0)
        for m in np.nonzero(p > around)[0]:
            lev = 10.0 * np.log10(self._five(int(m)) / ref) if self._five(int(m)) > 0.0 else -np.inf
            if m != m0 and lev >= threshold_db:
                out.append((float(d[m]), float(lev)))
        return [(0.0, 0.0)] + sorted(out)

    def outside_guard_db(self, cp):
        """10 log10 of the share of the profile's power whose delay relative to the strongest path lies outside [0, cp] samples -- by more than four bins
        (2.7 samples), the half width of the window's main lobe, which a path at 0 or at cp itself spreads over"""
        d, total = self.delays(), float(self.pdp.sum())
        outside = float(self.pdp[(d < -8.0 / 3.0 - 1e-9) | (d > cp + 8.0 / 3.0 + 1e-9)].sum())
        return 10.0 * np.log10(outside / total) if outside > 0.0 and total > 0.0 else -np.inf

    def ripple_db(self):
        """max over min of the amplitude response's power over the Kp carriers, in dB"""
        lo, hi = float(self.resp.min()), float(self.resp.max())
        return 10.0 * np.log10(hi / lo) if lo > 0.0 else np.inf
