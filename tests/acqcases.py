"""The streams and launches of tests/test_gpu_acquire.py and tests/test_acqref.py (a helper module, not a test file): every stream and every model run is built once per
process.  2k, guard 1/32 (L = 2112) unless a case says otherwise."""
import ctypes as C
import math

import numpy as np

import acqref

F = np.float32
FILL32 = np.frombuffer(b"\xa5" * 4, np.int32)[0]
LEAD_INS_ONE_PERIOD = [0, 1, 3, 7, 8, 9, 200, 2039, 2040]
LEAD_INS_TWO_PERIODS = [2047, 2048, 2111, 2112, 2115]
LOSSY_SNR_DB = 6.0                              # the reference's detector drops the lock every few dozen symbols
EPS_CEIL = 1e-6                                 # rad: epsilon is never allowed further from the float64 arctangent
EPS_FACTOR = 4.0                                # times what float32 arctan2 deviates over the same values: another libm, and float32 ulps near pi
PH_LINE_TOL = 5e-7                              # rad: one float32 ulp at pi plus the double sums
PH_HEAVY_TOL = 1e-5                             # rad: what tests/test_gpu_drift_kernels.py holds the accumulator's model to

_cache = {}


def cfg(po, mode=0, guard=0):
    return po.cfg(po.QPSK, po.C1_2, mode, guard)


def clean_stream(po, lead_in, npk=300, mode=0, guard=0, tail=None):
    """(cfg, samples): lead_in zeros, the symbols of npk packets, 3 N zeros"""
    key = ("clean", lead_in, npk, mode, guard, tail)
    if key not in _cache:
        c = cfg(po, mode, guard)
        _cache[key] = (c, po.tx(c, po.make_ts(npk, 17), lead_in=lead_in, tail=3 * c.N if tail is None else tail))
    return _cache[key]


def symbols(po, nsym, mode=0, guard=0):
    """exactly the first nsym OFDM symbols of the seeded stream, no lead-in, no tail"""
    key = ("symbols", mode, guard)
    c = cfg(po, mode, guard)
    per = c.payload * c.m * c.k // c.n                                # bits per symbol
    if key not in _cache or len(_cache[key]) < nsym * (c.N + c.cp):
        npk = (max(nsym, 64) + 16) * per // (188 * 8) + 24
        _cache[key] = po.tx(c, po.make_ts(npk, 17), lead_in=0, tail=0)
    x = _cache[key]
    assert len(x) >= nsym * (c.N + c.cp)
    return c, x[:nsym * (c.N + c.cp)]


def nsamples_for(c, ncalls):
    return (ncalls - 1) * (c.N + c.cp) + 2 * c.N + c.cp + 16


def eps_check(got, gammas):
    """(worst deviation of `got` from the float64 arctangent of the model's correlations, the same for float32 np.arctan2, the bound)"""
    gi = np.array([g[1] for g in gammas], F)
    gr = np.array([g[0] for g in gammas], F)
    want = np.arctan2(gi.astype(np.float64), gr.astype(np.float64))
    yard = float(np.abs(np.arctan2(gi, gr).astype(np.float64) - want).max()) if len(want) else 0.0
    worst = float(np.abs(np.asarray(got, F).astype(np.float64) - want).max()) if len(want) else 0.0
    return worst, yard, min(EPS_FACTOR * yard, EPS_CEIL)


def model(c, buf, nsamples, hist=0, avail=None, init_tries=4, carry=None, key=None):
    if key is not None and ("model", key) in _cache:
        return _cache[("model", key)]
    m = acqref.run_period(c.N, c.cp, buf, nsamples, hist, avail, 30.0, init_tries, carry)
    if key is not None:
        _cache[("model", key)] = m
    return m


def truncate(m, c, ncalls):
    """the model of the same stream cut to ncalls calls (a period whose windows never reach the cut: nothing it read changes)"""
    assert m["status"] == 0 and ncalls <= m["ncalls"]
    t = dict(m)
    t["ncalls"] = ncalls
    t["sym"] = m["sym"][:max(0, ncalls - m["call0"])]
    t["n_symbols"] = len(t["sym"])
    if len(t["sym"]) < len(m["sym"]) or not (m["status"] & 2):
        t["status"], t["lost_trk"], t["avg_lost"] = 0, None, m["avg"]
    return t


# ------------------------------------------------------------------------------------------------ the hook
CAP_2K, CAP_OTHER = 1200, 64                   # calls the handles hold: 2k guard 1/32 (the long cases), every other setting


def cap_calls(rx):
    N, cp = rx.dims.fft_length, rx.dims.cp_length
    return (rx.p.max_samples - (2 * N + cp + 16)) // (N + cp) + 1


def handle(g, mode, guard=0):
    """a receiver handle per (mode, guard), kept for the process"""
    key = ("rx", mode, guard)
    max_calls = CAP_2K if (mode, guard) == (0, 0) else CAP_OTHER
    if key not in _cache:
        N = 2048 if mode == 0 else 8192
        cp = N >> (5 - guard)
        _cache[key] = g.Rx(0, 0, mode, (max_calls - 1) * (N + cp) + 2 * N + cp + 16, guard=guard)
    return _cache[key]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def acquire(g, rx, buf, nsamples, hist=0, avail=None, init_tries=4, carry=None, path=0, force=0, nread=None, rows=True, expect=0):
    """dvbt_debug_acquire; returns dict(rep, meta (structured array), g_init, l_init, anchor_pos, centre, g_trk, l_trk) or the error code when `expect` is one"""
    N = rx.dims.fft_length
    buf = np.ascontiguousarray(buf, np.complex64)
    assert len(buf) >= hist + nsamples
    rep = g.binding.AcquireReport()
    ncalls = max(1, (nsamples - (2 * N + rx.dims.cp_length + 16)) // (N + rx.dims.cp_length) + 1)
    nread = min(ncalls + 8, cap_calls(rx)) if nread is None else nread
    meta = np.zeros(max(nread, 1), np.dtype([("cp_start", "<i4"), ("sw", "<i4"), ("eps", "<f4"), ("ph_base", "<f4"), ("incA", "<f8"), ("incB", "<f8")]))
    tries = min(init_tries, ncalls) if 1 <= init_tries <= 64 else 1
    out = {"g_init": np.zeros((tries, N), np.complex64), "l_init": np.zeros((tries, N), F), "init_flags": np.zeros((tries, N), np.uint8)}
    if rows:
        out.update(anchor_pos=np.zeros(cap_calls(rx) // 256 + 4, np.int32), centre=np.zeros(max(nread, 1), np.int32), g_trk=np.zeros((max(nread, 1), 32), np.complex64),
                   l_trk=np.zeros((max(nread, 1), 32), F))
    g.lib().dvbt_debug_acquire.argtypes = g.binding.ACQUIRE_ARGTYPES
    r = g.lib().dvbt_debug_acquire(rx.h, _p(buf), nsamples, hist, nsamples if avail is None else avail, init_tries, 0 if carry is None else 1,
                                   0.0 if carry is None else float(carry), path, force, C.byref(rep), _p(meta), nread, _p(out["g_init"]), _p(out["l_init"]),
                                   _p(out["anchor_pos"]) if rows else None, _p(out["centre"]) if rows else None, _p(out["g_trk"]) if rows else None,
                                   _p(out["l_trk"]) if rows else None, _p(out["init_flags"]))
    if expect:
        assert r == expect, (r, g.lib().dvbt_last_error())
        return r
    g.binding._chk(r)
    out.update(rep=rep, meta=meta[:nread], nread=nread)
    return out


ROUTES = ("general", "light", "heavy", "small")
_PATH_FORCE = {"general": (0, 0), "light": (0, 1), "heavy": (0, 2), "small": (1, 0)}


def route_taken(rep):
    """which kernels produced the result, from the flag words, small_viol and the walk counters"""
    if rep.small_passes:
        assert rep.general_passes == 0
        return "small_viol" if rep.small_viol else "small"
    assert rep.general_passes == 1
    if rep.need_heavy == 1:
        assert rep.need_seq == 1
        return "heavy"
    assert rep.need_heavy == 0
    if rep.need_seq == 1:
        return "light"
    assert rep.need_seq == 0
    return "general"


def wrap(x):
    return (x + math.pi) % (2 * math.pi) - math.pi


def check_search(m, got, name):
    """the initial windows the model examined: correlation and metric bit for bit, and the rise / keep decision of every sample -- acq_init_fsm_kernel forms the average
    in front of a sample from the 32 samples before it, the model by the plain recursion from the carried value"""
    avg = m["carry"]
    for t, rec in enumerate(m["init"]):
        assert got["l_init"][t].tobytes() == rec["lam"].tobytes(), (name, t)
        assert got["g_init"][t].real.tobytes() == rec["gr"].tobytes() and got["g_init"][t].imag.tobytes() == rec["gi"].tobytes(), (name, t)
        fl, avg = acqref.decisions(rec["lam"], avg)
        bad = np.flatnonzero(got["init_flags"][t] != fl)
        assert len(bad) == 0, (name, t, bad[:5], len(bad))
        assert avg.tobytes() == rec["avg_after"].tobytes()
    assert (got["init_flags"][len(m["init"]):] == 0xA5).all(), name  # windows behind the one that held the peak are not examined


def check(c, m, got, route, name=""):
    """the hook's results against the model m, bit for bit; `route`: the kernels the case was built for.  Returns the measured epsilon figures."""
    rep, meta, N, L = got["rep"], got["meta"], c.N, c.N + c.cp
    assert rep.ncalls == m["ncalls"]
    if m["status"] & 1:                                              # no peak in any window: status bit 0, nothing else written
        assert rep.status == 1 and rep.n_symbols == 0 and rep.call0 == 0 and rep.cp_start0 == 0, (rep.status, rep.n_symbols)
        assert np.float32(rep.avg).tobytes() == m["avg"].tobytes()
        assert (meta.view(np.int32) == FILL32).all()
        check_search(m, got, name)
        return None
    taken = route_taken(rep)
    if isinstance(route, tuple):
        assert taken in route, (name, taken, route)
        route = taken
    assert taken == route, (name, taken, route, list(rep.changed), rep.need_seq, rep.need_heavy, rep.small_viol)
    assert (rep.status, rep.call0, rep.cp_start0) == (m["status"] & ~2 if taken == "small_viol" else m["status"], m["call0"], m["cp_start0"]), \
        (name, rep.status, rep.call0, rep.cp_start0, rep.n_symbols, m["status"], m["call0"], m["cp_start0"], m["n_symbols"])
    assert np.float32(rep.avg).tobytes() == m["avg"].tobytes()
    check_search(m, got, name)
    got["taken"] = taken
    if taken == "small_viol":                                        # handed back to the host: nothing behind the initial search
        assert rep.n_symbols == 0 and (meta.view(np.int32) == FILL32).all()
        return None
    n = m["n_symbols"]
    assert rep.n_symbols == n, (name, rep.n_symbols, n)
    assert np.float32(rep.avg_lost).tobytes() == m["avg_lost"].tobytes(), (name, rep.avg_lost, m["avg_lost"])
    assert got["nread"] > n or got["nread"] == rep.cap_symbols
    assert (meta[n:].view(np.int32) == FILL32).all(), name           # nothing behind the last symbol is written
    want_cp = np.array([s["cp_start"] for s in m["sym"]], np.int32)
    want_sw = np.array([s["sw"] for s in m["sym"]], np.int32)
    assert (meta["cp_start"][:n] == want_cp).all(), (name, np.flatnonzero(meta["cp_start"][:n] != want_cp)[:5])
    assert (meta["sw"][:n] == want_sw).all(), name
    # the tracking metric of every lag the model evaluates, where the call's precomputed row holds it
    # (the rows that the walkers and acq_small_kernel compute on the spot are not exported: they are held to the model through cp_start, eps and the averages)
    if "l_trk" in got and route != "small":
        rows = 0
        track = m["sym"] + ([dict(lag0=m["lost_trk"]["stop"], **m["lost_trk"])] if m["lost_trk"] else [])
        for s, sym in enumerate(m["sym"] + ([dict(lag0=m["lost_trk"]["stop"], **m["lost_trk"])] if m["lost_trk"] else [])):
            call = m["call0"] + s
            if call >= got["nread"]:
                break
            rel0 = sym["lag0"] - (int(got["centre"][call]) - 16)
            if 0 <= rel0 <= 16:
                rows += 1
                assert got["l_trk"][call, rel0:rel0 + 16].tobytes() == sym["lam"].tobytes(), (name, s)
                assert got["g_trk"][call, rel0:rel0 + 16].real.tobytes() == sym["gr"].tobytes(), (name, s)
                assert got["g_trk"][call, rel0:rel0 + 16].imag.tobytes() == sym["gi"].tobytes(), (name, s)
        if route == "general":                                       # the placement stood: every call it examined lies inside its precomputed row
            assert rows == min(len(track), got["nread"] - m["call0"]) and (rows > 0 or not track), (name, rows, len(track))
        got["rows"] = rows
    # epsilon
    gam = [m["gamma_init"]] + [s["gamma"] for s in m["sym"]]
    eps = np.concatenate([[np.float32(rep.eps_init)], meta["eps"][:n]]).astype(F)
    worst, yard, bound = eps_check(eps, gam)
    assert worst <= bound, (name, worst, yard, bound)
    # the increments: exactly (-1 / N) (double)eps of the kernel's own estimates, one call apart
    if n:
        e = eps.astype(np.float64)
        incB = (-1.0 / N) * e[:n]
        assert (meta["incB"][:n] == incB).all(), name
        incA = np.zeros(n)
        for s in range(1, n):
            inside = 0 <= want_sw[s - 1] < L
            incA[s] = incB[s - 1] if inside or route != "heavy" else incA[s - 1]
        assert (meta["incA"][:n] == incA).all(), name
        if route == "heavy":
            lit = acqref.literal_phase(N, c.cp, eps[0], m["cp_start0"], want_cp, eps[1:])
            d = np.abs(wrap(meta["ph_base"][:n].astype(np.float64) - lit.astype(np.float64)))
            assert d.max() <= PH_HEAVY_TOL, (name, d.max())
        else:
            adv = [float(want_sw[s]) * incA[s] + float(L - want_sw[s]) * incB[s] for s in range(n)]
            line = np.array([math.fsum(adv[:s]) for s in range(n)]) if n <= 64 else np.concatenate([[0.0], _exact_cumsum(adv)[:-1]])
            d = np.abs(wrap(meta["ph_base"][:n].astype(np.float64) - line))
            assert d.max() <= PH_LINE_TOL, (name, d.max(), int(d.argmax()))
    return worst, yard


def _exact_cumsum(v):
    """running sums as math.fsum would give them: exact rational arithmetic on the doubles"""
    from fractions import Fraction
    acc, out = Fraction(0), []
    for x in v:
        acc += Fraction(x)
        out.append(float(acc))
    return np.array(out)


def run(g, c, rx, buf, nsamples, m, route, name="", **kw):
    path, force = _PATH_FORCE[route]
    got = acquire(g, rx, buf, nsamples, path=path, force=force, **kw)
    return check(c, m, got, route, name), got
