"""A plain float64 demodulator of one OFDM symbol, for the tests of the per-symbol kernels (a helper module, not a test file).

What symbol8k_kernel / symbol2k_kernel do to a symbol, stated in numpy: derotation by the acquisition's piecewise-linear phase, shifted FFT, the pilot engine of
reference_signals (integer offset, scattered-pilot pattern, LS gains, interpolation with the reference's constant 11, equalisation, channel state), nearest-point decision.
The same statements run in float32 (engine(..., np.float32) behind txref.fft32) give the error of a plain single-precision evaluation, which calibrates the bounds the
kernels are held to.  build_case makes the samples: carrier frames -> channel -> IFFT + cyclic prefix -> the inverse of the derotation, cast to complex64 ONCE, so that the
kernel and the reference read the same numbers.
"""
import ctypes as C

import numpy as np

import txref

_CT = {np.float32: np.complex64, np.float64: np.complex128}


class Tables:
    """pilot lists, w_k and the constellation of a configuration (po.cfg), from the oracle's generators"""

    def __init__(self, po, c):
        self.N, self.cp, self.zl, self.K, self.payload, self.m = c.N, c.cp, c.zeros_left, c.Kmax - c.Kmin + 1, c.payload, c.m
        wk = np.zeros(self.K, np.int8)
        po.lib().o_prbs_wk(C.byref(c), wk.ctypes.data_as(C.c_void_p))
        self.pilot = (4.0 * 2.0 * (0.5 - wk.astype(np.float64)) / 3.0)                      # +-4/3 at every carrier (used at the pilots only)
        self.cpilot = np.array([c.cpilot[i] for i in range(c.n_cpilot)], np.int64)
        self.tps = np.array([c.tps[i] for i in range(c.n_tps)], np.int64)
        d = self.pilot[self.cpilot[1:]] - self.pilot[self.cpilot[:-1]]
        self.known = d * d                                                                  # known_phase_diff
        self.n_spilot = c.n_spilot
        pts = np.zeros(c.csize, np.complex64)
        po.lib().o_constellation(C.byref(c), C.c_float(1.0), pts.ctypes.data_as(C.c_void_p))
        self.points = pts
        self.spacing = 2.0 * float(c.norm)
        self.c = c
        self._lists = {}

    def spilot(self, mod):
        size = self.n_spilot + (1 if mod == 0 else 0)
        k = 3 * (mod % 4) + 12 * np.arange(size)
        return k[k < self.K]

    def lists(self, mod):
        """(estimation carriers ascending, payload carriers) of pattern mod"""
        if mod not in self._lists:
            est = np.unique(np.concatenate([self.spilot(mod), self.cpilot]))
            pay = np.setdiff1d(np.arange(self.K), np.concatenate([est, self.tps]))
            assert len(pay) == self.payload and est[0] == 0 and est[-1] == self.K - 1
            self._lists[mod] = (est, pay)
        return self._lists[mod]


def phase64(N, cp, sw, ph_base, incA, incB):
    """the derotation phase of window sample n = 0 .. N - 1 (s8_fill_ptab and the pieceB test of the kernels): ph_base + (n + 1) incA up to the switch at sample count sw,
    incB beyond it; sw outside [0, N + cp): no switch"""
    n1 = np.arange(1, N + 1, dtype=np.float64)
    ph = float(ph_base) + n1 * float(incA)
    if 0 <= sw < N + cp:
        b = n1 > sw
        ph[b] = float(ph_base) + float(sw) * float(incA) + (n1[b] - float(sw)) * float(incB)
    return ph


def derotate64(x, N, cp, sw, ph_base, incA, incB, delta=None, dtype=np.float64):
    """window x[N] times expj(phase64), times (1 + i delta[n // 32]) with a drift table; dtype float32: the product in complex64 on a phasor rounded to complex64"""
    ct = _CT[dtype]
    y = np.asarray(x).astype(ct) * np.exp(1j * phase64(N, cp, sw, ph_base, incA, incB)).astype(ct)
    if delta is not None:
        y = y * (1 + 1j * np.repeat(np.asarray(delta, np.float64), 32)).astype(ct)
    return y.astype(ct)


def spectrum64(x):
    return np.fft.fftshift(np.fft.fft(np.asarray(x).astype(np.complex128)))


def _first_max_above_zero(v, default):
    v = np.where(np.isnan(v), -np.inf, v)
    i = int(np.argmax(v))                                      # the first of equal maxima: the strict > of the reference
    return i if v[i] > 0 else default


def engine(T, X, dtype=np.float64):
    """the pilot engine on one fft-shifted spectrum X[N] (oracle/o_demod.c::parse_input without the common phasor of frequency_correction, which cancels).
    Returns dict(fo, mod, eq[payload], tps[n_tps], csi[payload], gain[K])"""
    ft, ct = dtype, _CT[dtype]
    X = np.asarray(X).astype(ct)
    zl, K = T.zl, T.K
    pil, known = T.pilot.astype(ft), T.known.astype(ft)
    with np.errstate(all="ignore"):
        sums = np.empty(16, ft)
        for j, i in enumerate(range(zl - 8, zl + 8)):
            d = X[i + T.cpilot[1:]] - X[i + T.cpilot[:-1]]
            sums[j] = np.sum(known * (d.real * d.real + d.imag * d.imag), dtype=ft)
        fo = _first_max_above_zero(sums, 8) - 8
        x = X[zl + fo:zl + fo + K]                                 # carrier k
        pat = np.empty(4, ft)
        for s in range(4):
            k = T.spilot(s)[:10]
            acc = np.sum(pil[k].astype(ct) * np.conj(x[k]), dtype=ct)
            pat[s] = acc.real * acc.real + acc.imag * acc.imag
        mod = _first_max_above_zero(pat, 0)
        est, pay = T.lists(mod)
        g = pil[est].astype(ct) / x[est]
        gain = np.empty(K, ct)
        L = np.searchsorted(est, np.arange(K), side="right") - 1      # rank of the estimation carrier at or left of k
        L = np.minimum(L, len(est) - 2)
        j = (np.arange(K) - est[L]).astype(ft)
        tg = (g[L + 1] - g[L]) / ft(11.0)                             # the reference's constant, whatever the distance
        gain[:] = g[L] + tg * j
        gain[est] = g
        eq = (x[pay] * gain[pay]).astype(ct)
        tps = (x[T.tps] * gain[T.tps]).astype(ct)
        gp = gain[pay]
        csi = (ft(1.0) / (gp.real * gp.real + gp.imag * gp.imag)).astype(ft)
    return {"fo": fo, "mod": mod, "eq": eq, "tps": tps, "csi": csi, "gain": gain}


def decide64(T, eq):
    """(label of the nearest constellation point, each component's distance to the nearest decision boundary in units of the spacing [n][2]); the grid is a product of
    the levels of one axis, hierarchical alpha included, so the nearest point is the nearest level per axis"""
    p = T.points.astype(np.complex128)
    lv = np.unique(np.round(p.real / T.spacing * 2).astype(np.int64)) * (T.spacing / 2)      # levels (half spacings are exact integers of norm)
    bd = 0.5 * (lv[1:] + lv[:-1])
    ix = np.round(p.real / T.spacing * 2).astype(np.int64)
    iy = np.round(p.imag / T.spacing * 2).astype(np.int64)
    li = np.round(lv / T.spacing * 2).astype(np.int64)
    table = np.full((len(lv), len(lv)), -1, np.int64)
    table[np.searchsorted(li, ix), np.searchsorted(li, iy)] = np.arange(len(p))
    assert (table >= 0).all()
    e = np.asarray(eq).astype(np.complex128)
    comp = np.stack([e.real, e.imag], axis=-1)
    fin = np.isfinite(comp)
    cz = np.where(fin, comp, 0.0)
    cell = np.searchsorted(bd, cz)                                                            # level index per component
    dist = np.abs(cz[..., None] - bd).min(axis=-1) / T.spacing
    dist = np.where(fin, dist, 0.0)                                                           # a non-finite component is never "far from a boundary"
    return table[cell[..., 0], cell[..., 1]].astype(np.uint8), dist


def demap_rule(po, T, eq):
    """the reference's rule itself (o_demap: first strict minimum of the float distances over the point table) on complex64 values"""
    e = np.ascontiguousarray(eq, np.complex64).reshape(-1)
    out = np.zeros(e.size, np.uint8)
    po.lib().o_demap(C.byref(T.c), T.points.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_size_t(e.size))
    return out.reshape(np.shape(eq))


def two_echo(T):
    """H[b] on the fft-shifted grid of 1 + 0.3 z^(0.3 cp) + 0.2i z^(0.9 cp)"""
    f = (np.arange(T.N) - T.N // 2) / T.N
    d1, d2 = int(0.3 * T.cp), int(0.9 * T.cp)
    return 1 + 0.3 * np.exp(-2j * np.pi * f * d1) + 0.2j * np.exp(-2j * np.pi * f * d2)


class Case:
    """samples (complex64) + metadata of one launch, and its float64 / float32 references (computed once, on request)"""

    def __init__(self, T, iq, call0, cp_start, sw, ph_base, incA, incB, avail=None, delta=None):
        self.T, self.iq, self.call0 = T, iq, int(call0)
        n = len(cp_start)
        self.nsym = n
        self.cp_start = np.asarray(cp_start, np.int32)
        self.sw = np.broadcast_to(np.asarray(sw, np.int32), (n,)).copy()
        self.ph_base = np.broadcast_to(np.asarray(ph_base, np.float32), (n,)).copy()
        self.incA = np.broadcast_to(np.asarray(incA, np.float64), (n,)).copy()
        self.incB = np.broadcast_to(np.asarray(incB, np.float64), (n,)).copy()
        self.avail = (len(iq) if iq is not None else 0) if avail is None else int(avail)
        self.delta = None if delta is None else np.ascontiguousarray(delta, np.float32)
        self._ref = {}

    def moved(self, call0):
        """the same launch with its first samples cut off so that the state block's call0 is another: same windows, same references"""
        import copy
        o = copy.copy(self)
        o.iq = self.iq[(self.call0 - call0) * (self.T.N + self.T.cp):]
        o.avail = self.avail - (len(self.iq) - len(o.iq))
        o.call0 = int(call0)
        return o

    def low(self, s):
        return (self.call0 + s) * (self.T.N + self.T.cp) + int(self.cp_start[s]) - self.T.N + 1

    def window(self, s):
        """what the kernel's loads deliver: the N samples from low(s) on, zeros at or beyond avail"""
        N, a = self.T.N, self.low(s)
        assert a >= 0
        w = np.zeros(N, np.complex64)
        b = min(a + N, self.avail)
        if b > a:
            w[:b - a] = self.iq[a:b]
        return w

    def ref(self, dtype=np.float64, delta="own"):
        """dict of arrays over the symbols: acq, fft, eq, tps, csi, fo, mod"""
        key = (dtype, delta if isinstance(delta, str) else "none")
        if key not in self._ref:
            T = self.T
            out = {k: [] for k in ("acq", "fft", "eq", "tps", "csi", "fo", "mod")}
            for s in range(self.nsym):
                dl = self.delta[s] if (delta == "own" and self.delta is not None) else None
                a = derotate64(self.window(s), T.N, T.cp, int(self.sw[s]), self.ph_base[s], self.incA[s], self.incB[s], dl, dtype)
                X = spectrum64(a) if dtype == np.float64 else txref.fft32(a, True)
                e = engine(T, X, dtype)
                out["acq"].append(a); out["fft"].append(X)
                for k in ("eq", "tps", "csi", "fo", "mod"):
                    out[k].append(e[k])
            self._ref[key] = {k: np.array(v) for k, v in out.items()}
        return self._ref[key]


def build_case(T, freq, frames, H=None, shift=0, noise=0.0, seed=0, call0=0, inside=0, lead=0, sw=-1, ph_base=0.0, incA=0.0, incB=None, avail_cut=None, delta=None,
               tail=64):
    """frames: frame symbols (rows of freq, fft-shifted carriers, pilots 4/3) in any order, None = a symbol of zeros.  Every symbol goes through the channel H[N]
    (fft-shifted grid), an integer carrier shift and noise of standard deviation `noise` per carrier component, an IFFT, the cyclic prefix; the bodies lie on the regular
    grid body(s) = lead + cp + (call0 + s)(N + cp), and symbol s's window begins inside[s] samples in front of its body (inside the guard interval), which fixes cp_start;
    the body is advanced cyclically by as much, so the window holds the symbol itself wherever it begins (and something else if the kernel begins elsewhere).
    Then every window is rotated by the inverse of the derotation that (sw, ph_base, incA, incB), scalars or per symbol, describe.  avail_cut: samples cut from the END of
    the last window (avail = its end - avail_cut).  Everything in float64; one cast to complex64."""
    N, cp = T.N, T.cp
    n = len(frames)
    rng = np.random.RandomState(seed)
    inside = np.broadcast_to(np.asarray(inside, np.int64), (n,))
    shift = np.broadcast_to(np.asarray(shift, np.int64), (n,))
    incB = incA if incB is None else incB
    total = lead + cp + (call0 + n) * (N + cp) + tail
    buf = np.zeros(total, np.complex128)
    cp_start = np.empty(n, np.int32)
    for s, f in enumerate(frames):
        body = lead + cp + (call0 + s) * (N + cp)
        cp_start[s] = lead + cp - inside[s] + N - 1
        if f is None:
            continue
        X = np.asarray(f if not np.isscalar(f) else freq[f]).astype(np.complex128)
        if H is not None:
            X = X * H
        X = np.roll(X, int(shift[s]))
        if inside[s]:                                            # the window's head start is a cyclic delay of the body: taken out here, so that the equaliser's
            X = X * np.exp(2j * np.pi * (np.arange(N) - N // 2) * int(inside[s]) / N)   # interpolation (12 carriers wide) is not what such a launch measures
        if noise:
            X = X + noise * (rng.randn(N) + 1j * rng.randn(N))
        t = np.fft.ifft(np.fft.ifftshift(X))
        buf[body - cp:body] = t[N - cp:]
        buf[body:body + N] = t
    case = Case(T, None, call0, cp_start, sw, ph_base, incA, incB, delta=delta)
    for s in range(n):
        a = case.low(s)
        buf[a:a + N] *= np.exp(-1j * phase64(N, cp, int(case.sw[s]), case.ph_base[s], case.incA[s], case.incB[s]))
    case.iq = buf.astype(np.complex64)
    case.avail = len(case.iq) if avail_cut is None else case.low(n - 1) + N - int(avail_cut)
    return case


def worst(a, b):
    """largest |component difference| over the finite entries of b"""
    d = np.asarray(a).astype(np.complex128) - np.asarray(b).astype(np.complex128)
    ok = np.isfinite(np.asarray(b).astype(np.complex128))
    if not ok.any():
        return 0.0
    return float(max(np.abs(d.real[ok]).max(), np.abs(d.imag[ok]).max()))
