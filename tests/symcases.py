"""The launches of tests/test_gpu_symbol_kernels.py (a helper module, not a test file): built once per process, with their float64 and float32 references, so that the CPU
test of the reference (tests/test_symref.py) can hold every one of them to the conditions the GPU test relies on."""
import numpy as np

import symref

T2k, T8k = 0, 1
QPSK, QAM16, QAM64 = 0, 1, 2
F12 = list(range(8)) + [64, 65, 66, 67]                 # every pattern twice, the frame's last symbols
JUMPS = [0, 1, 2, 3, 4, 9, 10, 2, 2, 67, 0, 5]          # pattern jumps: the prediction cur_mod + (s - s_prev) is wrong at known places
SHIFTS = [-8, -3, 0, 7]
THREADS = {T2k: 128, T8k: 512}
CEIL = {"acq": 1e-6, "fft": 1e-5, "eq": 1e-3}           # the project's own ceilings (tests/test_gpu_chain.py): of the peak, of the peak, of the spacing
FACTOR = 8.0                                            # what the kernels legitimately do differently from a plain float32 evaluation
SHARE_CAP = 0.005                                       # components of a label comparison that may lie within the margin of a decision boundary

_tab, _cases = {}, {}


def tables(po, mode, const, hier=0, guard=0):
    """(symref.Tables, carrier frames of the first 68 symbols of a seeded stream)"""
    key = (mode, const, hier, guard)
    if key not in _tab:
        c = po.cfg(const, po.C1_2, mode, guard, hier)
        npk = 68 * (c.payload * c.m * c.k // c.n) // (204 * 8) + 2
        _, freq = po.tx(c, po.make_ts(npk, 31 + const), want_freq=True)
        assert len(freq) >= 68
        _tab[key] = (symref.Tables(po, c), freq[:68].astype(np.complex128))
    return _tab[key]


def sw_values(mode, N, cp):
    t = THREADS[mode]
    return [-1, 0, 1, 31, 32, 33, t - 1, t + 1, N // 2, N - 1, N, N + cp - 1, N + cp, 1 << 30]


def _seam_frame(T, frame, seed):
    """frame symbol 0 with payload carriers put ON the demapper's seams: a component at a decision boundary +- 0, 1e-6, 1e-5, 3e-5, 1e-4 cells (the cell test's margin, the
    four-candidate search's tie rule), others 3.9, 4.1 and 50 cells outside the grid (the exhaustive search)"""
    rng = np.random.RandomState(seed)
    X = frame.copy()
    _, pay = T.lists(0)
    lv = np.unique(np.round(T.points.real / T.spacing * 2).astype(np.int64)) * (T.spacing / 2)
    bd = 0.5 * (lv[1:] + lv[:-1])
    quiet = pay[(pay > 140) & (np.abs(pay[:, None] - T.cpilot[None, :]).min(axis=1) > 9)]      # (not where the two searches look: a carrier 50 cells out would outvote the pilots)
    pick = np.searchsorted(pay, rng.permutation(quiet)[:600])
    eps = np.array([0.0, 1e-6, -1e-6, 1e-5, -1e-5, 3e-5, -3e-5, 1e-4, -1e-4])
    far = np.array([3.9, 4.1, 50.0])
    for j, i in enumerate(pick):
        if j < 450:
            a = bd[rng.randint(len(bd))] + eps[j % len(eps)] * T.spacing
            b = bd[rng.randint(len(bd))] + eps[(j // len(eps)) % len(eps)] * T.spacing if j % 2 else lv[rng.randint(len(lv))] + 0.2 * T.spacing
        else:
            a = (lv[-1] + far[j % 3] * T.spacing) * (1 if j % 2 else -1)
            b = lv[rng.randint(len(lv))] + 0.1 * T.spacing if j % 4 < 2 else -(lv[-1] + far[(j // 3) % 3] * T.spacing)
        X[T.zl + pay[i]] = (a + 1j * b) if j % 3 else (b + 1j * a)
    return X


def _specs(mode):
    """name -> (constellation, hierarchy, guard, compares labels with decide64, builder(T, freq) -> symref.Case)"""
    N = 2048 if mode == T2k else 8192
    cfo = -2 * np.pi * 0.31 / N                                  # a carrier offset of 0.31 carrier spacings
    s = {}
    for const in (QPSK, QAM16, QAM64):
        for chan in ("flat", "echo"):
            s[f"taps_{const}_{chan}"] = (const, 0, 0, True, lambda T, f, chan=chan, const=const: symref.build_case(
                T, f, F12, H=symref.two_echo(T) if chan == "echo" else None, shift=[SHIFTS[i % 4] for i in range(12)], noise=0.01 if chan == "echo" else 0.0,
                seed=7 + const, ph_base=0.7, incA=cfo))
    s["jumps"] = (QAM16, 0, 0, True, lambda T, f: symref.build_case(T, f, JUMPS, H=symref.two_echo(T), noise=0.01, seed=3, ph_base=-1.1, incA=cfo))
    s["counts"] = (QAM16, 0, 0, True, lambda T, f: symref.build_case(T, f, [0, 1, 2, 3, 4, 5, 6, 7, 64], ph_base=0.2, incA=-cfo))
    for name, sgn in (("switch_up", 1.0), ("switch_down", -1.0)):
        s[name] = (QAM16, 0, 0, False, lambda T, f, sgn=sgn: symref.build_case(
            T, f, [i % 8 for i in range(14)], sw=sw_values(mode, T.N, T.cp), ph_base=0.4, incA=sgn * 2 * np.pi * 0.30 / T.N, incB=-sgn * 2 * np.pi * 0.45 / T.N))
    for guard in ((0, 1, 2, 3) if mode == T2k else (0, 3)):
        s[f"window_g{guard}"] = (QAM16, 0, guard, True, lambda T, f: symref.build_case(
            T, f, list(range(8)), call0=3, inside=[0, T.cp - 1, 1, T.cp // 2, T.cp // 2, 0, T.cp - 1, 1], ph_base=0.1, incA=cfo))
    s["drift"] = (QAM16, 0, 0, True, lambda T, f: symref.build_case(
        T, f, F12, H=symref.two_echo(T), noise=0.01, seed=5, ph_base=0.3, incA=cfo,
        delta=np.random.RandomState(9).uniform(-1.9e-3, 1.9e-3, (12, T.N // 32))))
    s["hier_16_a2"] = (QAM16, 2, 0, True, lambda T, f: symref.build_case(T, f, F12, H=symref.two_echo(T), noise=0.01, seed=11, ph_base=0.5, incA=cfo))
    s["hier_64_a4"] = (QAM64, 3, 0, True, lambda T, f: symref.build_case(T, f, F12, H=symref.two_echo(T), noise=0.01, seed=12, ph_base=0.5, incA=cfo))
    for const in (QPSK, QAM16, QAM64):
        s[f"seams_{const}"] = (const, 0, 0, False, lambda T, f, const=const: symref.build_case(
            T, f, [_seam_frame(T, f[0], 20 + const + k) for k in range(3)], ph_base=0.0, incA=0.0))
    return s


def names(mode):
    return list(_specs(mode)) + ["edge"]


def setting(mode, name):
    """(mode, constellation, hierarchy, guard) of a case's handle"""
    if name == "edge":
        name = "jumps"
    const, hier, guard, _, _ = _specs(mode)[name]
    return (mode, const, hier, guard)


def compares_labels(mode, name):
    return name != "edge" and _specs(mode)[name][3]


def case(po, mode, name):
    key = (mode, name)
    if key not in _cases:
        if name == "edge":
            _cases[key] = _edge(case(po, mode, "jumps"))
        else:
            const, hier, guard, _, build = _specs(mode)[name]
            T, freq = tables(po, mode, const, hier, guard)
            _cases[key] = build(T, freq)
    return _cases[key]


EDGE_ZERO, EDGE_CUT = 3, (9, 10, 11)


def _edge(base):
    """the end of the memory, from the launch `jumps`: symbol 3 is all zeros; avail lies one sample in front of symbol 9's last one, symbol 10's window is moved so that
    its second half lies beyond avail, symbol 11's lies wholly beyond it.  The other symbols read what they read in `jumps`."""
    import copy
    T = base.T
    N = T.N
    c = copy.copy(base)
    c._ref = {}
    c.iq = base.iq.copy()
    c.cp_start = base.cp_start.copy()
    a = base.low(EDGE_ZERO)
    c.iq[a:a + N] = 0
    c.avail = base.low(9) + N - 1
    c.cp_start[10] += (c.avail - N // 2) - base.low(10)
    for k in ("sw", "ph_base", "incA", "incB"):
        getattr(c, k)[10] = getattr(base, k)[9]
    assert c.low(10) + N // 2 == c.avail and c.low(11) >= c.avail and c.low(8) + N <= c.avail
    return c


def bounds(po, mode):
    """the working bounds of a mode: FACTOR times the largest error of the float32 evaluation against the float64 one over the module's launches, never above the project's
    ceiling: acq and fft in units of the launch's peak, eq and tps in units of the spacing, csi relative"""
    key = (mode, "bounds")
    if key not in _cases:
        w = {"acq": 0.0, "fft": 0.0, "eq": 0.0, "tps": 0.0, "csi": 0.0}
        for name in names(mode):
            if name == "edge" or name.startswith("seams"):       # (a symbol cut in half has pilots near zero: its carriers are held to these bounds where float32 itself
                continue                                         # meets them; the seams' launches, with carriers 50 cells out, compare no tap within a bound)
            c = case(po, mode, name)
            r, r32 = c.ref(np.float64), c.ref(np.float32)
            same = (r["fo"] == r32["fo"]) & (r["mod"] == r32["mod"])
            assert same.all(), (mode, name)
            for k in ("acq", "fft"):
                w[k] = max(w[k], symref.worst(r32[k], r[k]) / np.abs(r[k]).max())
            for k in ("eq", "tps"):
                w[k] = max(w[k], symref.worst(r32[k], r[k]) / c.T.spacing)
            ok = np.isfinite(r["csi"]) & (r["csi"] > 0)
            with np.errstate(all="ignore"):
                w["csi"] = max(w["csi"], float(np.abs(r32["csi"][ok].astype(np.float64) / r["csi"][ok] - 1).max()) if ok.any() else 0.0)
        b = {k: FACTOR * v for k, v in w.items()}
        for k, ceil in CEIL.items():
            b[k] = min(b[k], ceil)
        _cases[key] = (b, w)
    return _cases[key][0]


def float32_errors(po, mode):
    bounds(po, mode)
    return _cases[(mode, "bounds")][1]
