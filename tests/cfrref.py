"""The crest-factor reduction block's specification (include/dvbt_hip.h, dvbt_cfr_*) in numpy, complex128: iterative clipping and filtering of whole OFDM
symbols.  Step numbers are the header's.  Nothing here knows the GPU library."""
import numpy as np

KEEP_PILOTS, KEEP_TPS = 1, 2
FIELDS = ("symbols", "symbols_clipped", "symbols_nonfinite", "samples_over", "peak_power_in")

# ETSI EN 300 744 tables 7 and 8, 2k mode; 8k repeats them with period 1704 and adds the last continual pilot
_CPILOT_2K = (0, 48, 54, 87, 141, 156, 192, 201, 255, 279, 282, 333, 432, 450, 483, 525, 531, 618, 636, 714, 759, 765, 780, 804, 873, 888, 918, 939, 942,
              969, 984, 1050, 1101, 1107, 1110, 1137, 1140, 1146, 1206, 1269, 1323, 1377, 1491, 1683, 1704)
_TPS_2K = (34, 50, 209, 346, 413, 569, 595, 688, 790, 901, 1073, 1219, 1262, 1286, 1469, 1594, 1687)


class Mode:
    """the sizes and carrier lists of a transmission mode (0: 2k, 1: 8k) and guard interval (0 .. 3: 1/32 .. 1/4)"""

    def __init__(self, mode, guard):
        self.N = 8192 if mode else 2048
        self.G = self.N // (32, 16, 8, 4)[guard]
        self.K = 6817 if mode else 1705
        self.half = (self.K - 1) // 2
        self.cpilot = np.array(_CPILOT_2K if not mode else [k + 1704 * r for r in range(4) for k in _CPILOT_2K[:44]] + [6816])
        self.tps = np.array([k + 1704 * r for r in range(4 if mode else 1) for k in _TPS_2K])
        k = np.arange(self.N)
        self.kappa = np.where(k < self.N // 2, k, k - self.N)             # step 1: the signed index of bin k
        self.occupied = np.abs(self.kappa) <= self.half
        self.carrier = self.kappa + self.half                             # meaningful on the occupied bins

    @property
    def symbol(self):
        return self.G + self.N

    def bins(self, carriers):
        """the bins of a list of carriers"""
        return (np.asarray(carriers) - self.half) % self.N

    def scattered(self, l):
        return np.arange(3 * (l % 4), self.K, 12)

    def kept(self, l, keep):
        """step 5: the carriers of symbol l whose error is zeroed"""
        parts = [np.zeros(0, np.int64)]
        if keep & KEEP_PILOTS:
            parts += [self.cpilot, self.scattered(l)]
        if keep & KEEP_TPS:
            parts.append(self.tps)
        return np.unique(np.concatenate(parts))

    def free(self, l, keep):
        """boolean per bin: where the filter lets the clipping error through"""
        f = self.occupied.copy()
        f[self.bins(self.kept(l, keep))] = False
        return f


def rotation(md, p, os):
    """step 2: r_p[k] = e^{2 pi i kappa p / (os N)}"""
    return np.exp(2j * np.pi * md.kappa * p / (os * md.N))


def phases(md, X, os):
    """step 2: x_p[n], rows p < os"""
    return np.stack([np.fft.ifft(X * rotation(md, p, os)) for p in range(os)])


def clip(x, A):
    """step 3"""
    m = np.abs(x)
    return np.where(m > A, x * (A / np.where(m > 0, m, 1.0)), x)


def back(md, c, os):
    """step 4: C[k] from the clipped phases (rows)"""
    return sum(np.fft.fft(c[p]) * np.conj(rotation(md, p, os)) for p in range(os)) / os


def threshold_for(papr_db, ref_power):
    return float(np.sqrt(ref_power * 10.0 ** (papr_db / 10.0)))


def new_counters():
    return dict(symbols=0, symbols_clipped=0, symbols_nonfinite=0, samples_over=0, peak_power_in=0.0, margin=np.inf)


def run_symbol(md, sym, l, A, iterations, os, keep, ctr=None):
    """one symbol of G + N samples, index l in the stream's frame.  ctr (new_counters) accumulates the header's five and `margin`, the smallest
    | |x_p[n]| - A | / A of a first iteration: how far the counters are from depending on rounding."""
    ctr = new_counters() if ctr is None else ctr
    sym = np.asarray(sym)
    assert sym.shape == (md.symbol,)
    ctr["symbols"] += 1
    if not np.isfinite(sym.view(np.float32 if sym.dtype == np.complex64 else np.float64)).all():
        ctr["symbols_nonfinite"] += 1
        return sym.copy()
    if iterations == 0:
        return sym.copy()
    X0 = np.fft.fft(sym[md.G:].astype(np.complex128))
    free = md.free(l, keep)
    X = X0.copy()
    for it in range(iterations):
        x = phases(md, X, os)
        if it == 0:
            m = np.abs(x)
            ctr["peak_power_in"] = max(ctr["peak_power_in"], float((m * m).max()))
            ctr["margin"] = min(ctr["margin"], float(np.abs(m - A).min() / A))
            n_over = int((m > A).sum())
            if n_over == 0:
                return sym.copy()
            ctr["symbols_clipped"] += 1
            ctr["samples_over"] += n_over
        E = np.where(free, back(md, clip(x, A), os) - X0, 0.0)            # step 5
        X = X0 + E
    u = np.fft.ifft(X)
    return np.concatenate([u[md.N - md.G:], u])


def run(md, iq, A, iterations=4, os=2, keep=KEEP_PILOTS | KEEP_TPS, first_symbol=0, ctr=None):
    """a stream of whole symbols -> (complex128 output, counters)"""
    ctr = new_counters() if ctr is None else ctr
    iq = np.asarray(iq)
    assert len(iq) % md.symbol == 0
    rows = iq.reshape(-1, md.symbol)
    out = [run_symbol(md, rows[l], first_symbol + l, A, iterations, os, keep, ctr) for l in range(len(rows))]
    return (np.concatenate(out).astype(np.complex128) if out else np.zeros(0, np.complex128)), ctr


# ------------------------------------------------------------------ instruments for the tests
def interpolated_peak_db(md, iq, ref_power, factor=8):
    """the highest |x|^2 of each symbol's useful part interpolated `factor` times (zero-padded spectrum), in dB over ref_power: one figure per symbol"""
    rows = np.asarray(iq, np.complex128).reshape(-1, md.symbol)[:, md.G:]
    X = np.fft.fft(rows, axis=1)
    Z = np.zeros((len(rows), factor * md.N), np.complex128)
    Z[:, :md.N // 2] = X[:, :md.N // 2]
    Z[:, -md.N // 2:] = X[:, md.N // 2:]
    z = np.fft.ifft(Z, axis=1) * factor
    return 10.0 * np.log10((np.abs(z) ** 2).max(axis=1) / ref_power)


def synthetic_symbols(md, nsym, seed, first_symbol=0, scale=1.0):
    """QAM64 of unit power on the data carriers, pilots (continual and scattered) at +-4/3, TPS at +-1, nothing outside the band: complex64 with prefix"""
    rng = np.random.RandomState(seed)
    lev = np.arange(-7, 8, 2) / np.sqrt(42.0)
    out = []
    for l in range(nsym):
        c = rng.choice(lev, md.K) + 1j * rng.choice(lev, md.K)
        pil = np.unique(np.concatenate([md.cpilot, md.scattered(first_symbol + l)]))
        c[pil] = (4.0 / 3.0) * rng.choice((-1.0, 1.0), len(pil))
        c[md.tps] = rng.choice((-1.0, 1.0), len(md.tps))
        X = np.zeros(md.N, np.complex128)
        X[md.bins(np.arange(md.K))] = c
        u = np.fft.ifft(X) * scale * md.N / np.sqrt(md.K)
        out.append(np.concatenate([u[md.N - md.G:], u]))
    return np.concatenate(out).astype(np.complex64)


def papr_db(iq, prob):
    """the level in dB over the mean power that |x|^2 exceeds with probability prob"""
    p = np.abs(np.asarray(iq, np.complex128)) ** 2
    return float(10.0 * np.log10(np.quantile(p, 1.0 - prob) / p.mean()))
