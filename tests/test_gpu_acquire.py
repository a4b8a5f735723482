"""The acquisition kernels of gr_dvbt_amd/csrc/k_frontend.hpp ALONE (dvbt_debug_acquire: a test hook of the library that runs launch_acquisition, the segment path's own
launch routine), where the chain tests reach them only through a whole receiver and compare cp_start.  The reference is tests/acqref.py, a literal float32 model of
the reference block that tests/test_acqref.py pins against oracle/o_acq.c on the CPU.  Compared bit for bit: status, call0, cp_start0, n_symbols, every cp_start and
switch position, the initial windows' correlation and metric, the tracking metric of every lag the model evaluates (where the call's precomputed row holds it), the
detector's average behind the search and behind a lost lock.  Epsilon: against the float64 arctangent of the model's correlation, within 4 times what float32
np.arctan2 deviates over the same values, never above 1e-6 rad.  The increments: exactly (-1 / N) (double)eps of the kernel's own estimates.  The entry phase: on the
line routes within 5e-7 rad of the exactly summed line of the kernel's own increments, on the float-faithful walk within 1e-5 rad of the literal accumulator.

Every case names the route it was built for -- the Jacobi placement with acq_finalize_kernel ("general"), the light walk, the float-faithful heavy walk,
acq_small_kernel -- and fails if the flag words, small_viol and the walk counters say another one produced the result.  Every buffer the kernels write is 0xA5 before
the launches: the SymMeta rows behind n_symbols must still be."""
import numpy as np
import pytest

import gr_dvbt_amd as g

import acqcases as ac

pytestmark = pytest.mark.gpu
L2K = 2112


def routes_for(m, c, ncalls, routes=ac.ROUTES):
    """(route asked for, route expected): a period with a switch position outside its call goes to the heavy walk whatever was asked, and acq_small_kernel hands it back"""
    Lc = c.N + c.cp
    viol = any(s["sw"] < 0 or s["sw"] >= Lc for s in m["sym"])
    out = []
    for r in routes:
        if r == "small" and ncalls > 768:
            continue
        out.append((r, ("small_viol" if r == "small" else "heavy") if viol else r))
    return out


def run_all(c, rx, buf, nsamples, m, name, routes=ac.ROUTES, natural=None, **kw):
    """every route on one stream; all must match the model (hence each other).  natural: the route the general kernels take by themselves, where it is not the placement"""
    figs = []
    for asked, want in routes_for(m, c, m["ncalls"], routes):
        if natural and asked == "general" and want == "general":
            want = PINNED[name] if natural == "table" else natural
        path, force = ac._PATH_FORCE[asked]
        got = ac.acquire(g, rx, buf, nsamples, path=path, force=force, **kw)
        f = ac.check(c, m, got, want, f"{name}/{asked}")
        if f:
            figs.append(f)
    if figs:
        worst, yard = max(f[0] for f in figs), max(f[1] for f in figs)
        print(f"\n[{name}] {m['ncalls']} calls, {m['n_symbols']} symbols from call {m['call0']}, status {m['status']}; epsilon worst {worst:.3e} rad, float32 arctan2 {yard:.3e}"
              + (f" ({worst / yard:.2f} x)" if yard else ""))


# Which kernels produce the result when nothing is forced, for the streams on which that is not the placement by construction.  It hangs on the anchors: one that
# falls into the dead part of a stream reports whatever lag holds the largest metric there (silence: the window's first lag, 200 from cp_start0, accepted, and the centres
# leave the tracker within a dozen calls; noise: anywhere).  Deterministic per stream, recorded from the MI355X and asserted.
PINNED = {
    'equal peaks': 'general',
    'plus1 x4': 'general',
    'lost at 1 noise': 'general',
    'lost at 1 zeros': 'general',
    'lost at 2 noise': 'general',
    'lost at 2 zeros': 'general',
    'lost at 3 noise': 'general',
    'lost at 3 zeros': 'general',
    'lost at 17 noise': 'general',
    'lost at 17 zeros': 'light',
    'lost at 242 noise': 'light',
    'lost at 242 zeros': 'light',
    'lost at 243 noise': 'light',
    'lost at 243 zeros': 'light',
    'lost at 244 noise': 'general',
    'lost at 244 zeros': 'light',
    'lost at 245 noise': 'general',
    'lost at 245 zeros': 'light',
    'lost at 1022 noise': 'general',
    'lost at 1022 zeros': 'light',
    'lost at 1023 noise': 'light',
    'lost at 1023 zeros': 'light',
    'lost at 1024 noise': 'light',
    'lost at 1024 zeros': 'light',
    'lost at 1098 noise': 'general',
    'lost at 1098 zeros': 'general',
}


@pytest.fixture(scope="module")
def static(po):
    """200 zeros, 1104 symbols, a carrier offset of 0.11 spacings (no noise: the position never moves, epsilon and the phase line are not zero); the model of its
    first 1100 calls"""
    c, x = ac.symbols(po, 1104)
    buf = po.channel(np.concatenate([np.zeros(200, np.complex64), x]), c.N, cfo=0.11)
    n = ac.nsamples_for(c, 1100)
    assert n <= len(buf)
    return c, buf, ac.model(c, buf, n, key="static1100")


# ------------------------------------------------------------------------------------------------ a static clean stream, every route
@pytest.mark.parametrize("ncalls", [5, 243, 244, 245, 488, 489, 768, 1023, 1024, 1025, 1100])
def test_static_stream_every_route(static, ncalls):
    """around the 244 calls a workgroup of acq_track_fused_kernel owns, the 1024 of acq_finalize_kernel, ACQ_SMALL_MAX_CALLS"""
    c, buf, m1100 = static
    assert m1100["n_symbols"] == 1100 and m1100["cp_start0"] == 2311
    run_all(c, ac.handle(g, 0), buf, ac.nsamples_for(c, ncalls), ac.truncate(m1100, c, ncalls), f"static {ncalls}")


@pytest.mark.parametrize("mode,guard", [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 3)])
def test_every_guard_interval(po, mode, guard):
    """cp up to ACQ_CP_MAX: the span clamp of acq_metric_kernel's last workgroup, acq_small_cpc at both clamps; with a carrier offset, so that epsilon is not 0"""
    c, x = ac.symbols(po, 44, mode, guard)
    buf = po.channel(np.concatenate([np.zeros(300, np.complex64), x]), c.N, cfo=0.23, snr_db=35.0, seed=3, ref_span=(1000, 60000))
    n = ac.nsamples_for(c, 40)
    m = ac.model(c, buf, n)
    assert m["status"] == 0 and m["n_symbols"] >= 30
    run_all(c, ac.handle(g, mode, guard), buf, n, m, f"mode {mode} guard {guard}")


# ------------------------------------------------------------------------------------------------ the initial search
@pytest.mark.parametrize("lead_in", [255, 256, 2039, 2040, 2047, 2048, 2111, 2112, 2115])
def test_peak_position_in_the_first_window(po, lead_in):
    """the peak at lags 255, 256, N - 9, N - 8; at N - 1 and behind the window: an open peak is not counted, the lock found instead is dropped within a call or two"""
    c, x = ac.symbols(po, 30)
    buf = np.concatenate([np.zeros(lead_in, np.complex64), x])
    n = ac.nsamples_for(c, 24)
    m = ac.model(c, buf, n)
    if lead_in <= 2040:
        assert m["cp_start0"] == 2111 + lead_in and m["n_symbols"] == 24
    else:
        assert m["status"] & 2 and m["n_symbols"] <= 1
    run_all(c, ac.handle(g, 0), buf, n, m, f"lead-in {lead_in}")


@pytest.mark.parametrize("silent,tries", [(1, 1), (1, 4), (3, 4), (4, 4), (4, 5), (4, 64), (3, 64)])
def test_silent_windows_and_init_tries(po, silent, tries):
    """silence in the first windows: the search goes on to the next one while it has tries, and writes nothing but status bit 0 when it runs out"""
    c, x = ac.symbols(po, 30)
    buf = np.concatenate([np.zeros((silent - 1) * L2K + 2 * c.N + c.cp + 100, np.complex64), x])    # windows 0 .. silent - 1 see nothing at all
    n = ac.nsamples_for(c, 24)
    m = ac.model(c, buf, n, init_tries=tries)
    assert (m["status"] & 1) == (1 if tries <= silent else 0) and (m["status"] & 1 or m["call0"] >= silent)
    run_all(c, ac.handle(g, 0), buf, n, m, f"silent {silent} tries {tries}", routes=("general", "small"), init_tries=tries)


@pytest.mark.parametrize("carry", [0.0, 37.5, 1e7, -5.0, 1e30])
def test_carried_average(po, carry):
    """d_avg carried in from the call that lost the previous lock: a large one holds the detector down until it has decayed (0.1 per sample)"""
    c, x = ac.symbols(po, 30)
    buf = po.channel(np.concatenate([np.zeros(700, np.complex64), x]), c.N, snr_db=20.0, seed=4, ref_span=(1000, 60000))
    n = ac.nsamples_for(c, 24)
    m = ac.model(c, buf, n, carry=carry)
    run_all(c, ac.handle(g, 0), buf, n, m, f"carry {carry}", routes=("general", "small"), carry=carry)


def test_noisy_windows_pin_the_restarted_average(po):
    """noise alone in every window: thousands of rise / keep decisions per window hang on the average that acq_init_fsm_kernel restarts 32 samples back; the metric of
    all windows, every sample's rise / keep decision, the verdict (no peak in any window) and the average behind the last window must be the sequential model's"""
    c = ac.cfg(po)
    rng = np.random.RandomState(21)
    buf = (rng.randn(ac.nsamples_for(c, 8)) + 1j * rng.randn(ac.nsamples_for(c, 8))).astype(np.complex64)
    for tries in (1, 5):
        m = ac.model(c, buf, len(buf), init_tries=tries)
        assert m["status"] == 1 and len(m["init"]) == tries
        run_all(c, ac.handle(g, 0), buf, len(buf), m, f"noise tries {tries}", routes=("general", "small"), init_tries=tries)


def test_equal_peaks_first_wins(po):
    """a stream of period 512: x[i] == x[i - N] everywhere, the metric repeats every 512 lags bit for bit, so every peak of a window has three exact equals; the
    reference takes the first of the largest"""
    c = ac.cfg(po)
    rng = np.random.RandomState(5)
    block = ((rng.randn(512) + 1j * rng.randn(512)) * np.where((np.arange(512) > 200) & (np.arange(512) < 300), 3.0, 0.3)).astype(np.complex64)   # a burst per period
    n = ac.nsamples_for(c, 8)
    buf = np.tile(block, n // 512 + 1)[:n]
    m = ac.model(c, buf, n)
    lam = m["init"][0]["lam"]
    assert m["status"] != 1 and m["call0"] == 0 and lam[:512].tobytes() == lam[512:1024].tobytes() == lam[1536:2048].tobytes()
    assert m["cp_start0"] - 2111 < 512 and (lam == lam[m["cp_start0"] - 2111]).sum() >= 4
    run_all(c, ac.handle(g, 0), buf, n, m, "equal peaks", routes=("general", "small"), natural="table")


@pytest.mark.parametrize("which", [1, 2])
def test_rejected_anchor(po, which):
    """a burst in the window of an anchor's call, 1,000 lags from the tracked peak and outside every sample the tracker reads: the anchor reports it, acq_centre_kernel
    rejects it (further from the last accepted one than a sample per call), interpolates across it (anchor 1) or extrapolates from the two before (anchor 2, the
    last), the centres stay on the peak and the placement stands"""
    c, x = ac.symbols(po, 604)
    buf = np.concatenate([np.zeros(600, np.complex64), x])
    n = ac.nsamples_for(c, 600)
    at = which * 256 * L2K
    buf[at + 3648:at + 3712] = 12.0 * np.abs(x[:4096]).std() * (1 + 1j)        # lag 3711: the samples 3648 .. 3711 and the same N earlier
    buf[at + 1600:at + 1664] = buf[at + 3648:at + 3712]
    m = ac.model(c, buf, n)
    assert m["status"] == 0 and m["n_symbols"] == 600 and m["cp_start0"] == 2711 and all(s["cp_start"] == 2711 for s in m["sym"])
    run_all(c, ac.handle(g, 0), buf, n, m, f"rejected anchor {which}", routes=("general", "small"))
    got = ac.acquire(g, ac.handle(g, 0), buf, n)
    assert abs(int(got["anchor_pos"][which]) - 3711) <= 2 and got["anchor_pos"][3 - which] == 2711
    assert (got["centre"][:600] == 2711).all()


def test_window_creeps_past_the_forecast(po):
    """five samples more per call for 380 calls: cp_start passes 2N + cp - 2 = 4158, the window reads beyond its call's 2N + cp + 16 samples (the stream's own, zeros
    beyond avail), the anchors cannot see the peak any more"""
    gaps = {s: 5 for s in range(5, 385)}
    c, buf = respaced(po, 405, gaps)
    n = ac.nsamples_for(c, 400)
    m = ac.model(c, buf[:n], n)
    assert m["n_symbols"] >= 390 and max(s["cp_start"] for s in m["sym"]) > 2 * c.N + c.cp - 2 + 40, (m["status"], m["n_symbols"])
    run_all(c, ac.handle(g, 0), buf[:n], n, m, "creep", natural="light")


# ------------------------------------------------------------------------------------------------ the stream's left edge
@pytest.mark.parametrize("lead_in", range(10))
def test_stream_begins_at_a_symbol_start(po, lead_in):
    """the first tracking window (cp_start0 - 8 ..) reaches in front of the stream's first sample: the taps whose partner does not exist are skipped, as the reference's
    restatement skips them, and the lock holds.  Lead-in 0 has sw = -1 at call 0: the float-faithful walk's own territory"""
    c, x = ac.symbols(po, 40)
    buf = np.concatenate([np.zeros(lead_in, np.complex64), x])
    n = ac.nsamples_for(c, 30)
    m = ac.model(c, buf, n)
    assert m["status"] == 0 and m["cp_start0"] == 2111 + lead_in and m["n_symbols"] == 30 and m["sym"][0]["sw"] == lead_in - 1
    run_all(c, ac.handle(g, 0), buf, n, m, f"lead-in {lead_in}")


@pytest.mark.parametrize("hist", [4, 8, 40])
@pytest.mark.parametrize("lead_in", [0, 1, 3, 7, 8, 9])
def test_segment_begins_at_a_symbol_start_with_history(po, lead_in, hist):
    """the same inside a stream: `hist` real samples lie in front of the segment, the window reads them; what lies further back does not exist"""
    c, x = ac.symbols(po, 44)
    cut = 3 * L2K - lead_in - hist                                    # the segment begins lead_in samples in front of symbol 3
    buf = x[cut:]
    n = ac.nsamples_for(c, 30)
    m = ac.model(c, buf, n, hist=hist)
    assert m["status"] == 0 and m["n_symbols"] >= 1
    run_all(c, ac.handle(g, 0), buf, n, m, f"lead-in {lead_in} hist {hist}", hist=hist)


# ------------------------------------------------------------------------------------------------ the right edge
@pytest.mark.parametrize("short", [-1, 0, 1, 9, 80, 2112])
def test_avail_at_the_last_window(static, short):
    """avail one sample beyond, at and inside the last tracking window, and further in: samples at or beyond it read as zeros though the buffer holds others"""
    c, buf, _ = static
    ncalls = 30
    n = ac.nsamples_for(c, ncalls)
    avail = (ncalls - 1) * L2K + 2311 + 8 - short
    junk = buf[:n].copy()
    junk[avail:] = 3.0 - 2.0j
    m = ac.model(c, junk, n, avail=avail)
    assert m["status"] in (0, 2)
    run_all(c, ac.handle(g, 0), junk, n, m, f"avail short {short}", avail=avail)


# ------------------------------------------------------------------------------------------------ a symbol spacing that changes
def respaced(po, nsym, gaps, lead_in=200):
    """the stream with gaps[s] samples inserted in front of symbol s (zeros), or -gaps[s] samples of its guard interval dropped"""
    c, x = ac.symbols(po, nsym)
    sym = x.reshape(nsym, c.N + c.cp)
    parts = [np.zeros(lead_in, np.complex64)]
    for s in range(nsym):
        d = gaps.get(s, 0)
        parts.append(np.zeros(d, np.complex64) if d > 0 else np.zeros(0, np.complex64))
        parts.append(sym[s][max(0, -d):])
    return c, np.concatenate(parts)


SPACING = {
    "plus1 x3": ({s: 1 for s in range(10, 13)}, "general"),           # three moves: the four Jacobi rounds settle
    "plus1 x4": ({s: 1 for s in range(10, 14)}, None),
    "plus1 x5": ({s: 1 for s in range(10, 15)}, "general"),           # (a peak up to 6 lags off the first one is inside every round's window: still settled)
    "plus1 x9": ({s: 1 for s in range(10, 19)}, "light"),             # nine in a row: the rounds gain a call each and do not settle
    "plus7": ({10: 7}, "general"),                                    # the peak at the window's last lag is still open at its end: not counted, the lock is lost
    "minus7": ({10: -7}, "general"),
    "plus6": ({10: 6}, "light"),                                      # (round 0 sees the moved peak at its window's edge with another average: open, and so on down the calls)
    "plus6 minus6": ({10: 6, 20: -6, 21: -6, 30: 6}, "light"),
    "ramp 12": ({s: 1 for s in range(8, 20)}, "light"),               # more than R - 8 from the centre: direct rows in every walker
    "ramp -12": ({s: -1 for s in range(8, 20)}, "light"),
}


@pytest.mark.parametrize("name", list(SPACING))
def test_symbol_spacing_changes(po, name):
    gaps, natural = SPACING[name]
    c, buf = respaced(po, 48, gaps)
    n = ac.nsamples_for(c, 40)
    m = ac.model(c, buf, n)
    moved = sum(gaps.values())
    if name == "plus7":
        assert m["status"] == 2 and m["n_symbols"] == 10
    else:
        assert m["status"] == 0 and m["n_symbols"] == 40 and m["sym"][-1]["cp_start"] == 2311 + moved, (m["status"], m["n_symbols"])
    run_all(c, ac.handle(g, 0), buf, n, m, name, natural=natural or "table")   # (four moves: what the rounds did with it is in the table)


def test_slow_drift_across_three_anchors(po):
    """one sample every 30 calls over 800 calls: the anchors follow, the centres interpolate, the placement settles"""
    gaps = {s: 1 for s in range(20, 800, 30)}
    c, buf = respaced(po, 812, gaps)
    n = ac.nsamples_for(c, 800)
    m = ac.model(c, buf, n)
    assert m["status"] == 0 and m["n_symbols"] == 800 and m["sym"][-1]["cp_start"] == 2311 + len(gaps)
    run_all(c, ac.handle(g, 0), buf, n, m, "slow drift", routes=("general", "light", "heavy"), natural="light")   # (the placement's rounds all start from cp_start0)


# ------------------------------------------------------------------------------------------------ a lost lock
@pytest.mark.parametrize("fill", ["zeros", "noise"])
@pytest.mark.parametrize("call", [1, 2, 3, 17, 242, 243, 244, 245, 1022, 1023, 1024, 1098])
def test_lost_lock(static, call, fill):
    """the stream ends in front of call `call`'s window (zeros to the end, or zeros for a call and a half and then noise): n_symbols, status bit 1, the average the
    reference would re-acquire with, the rows behind n_symbols untouched, on every route.  Which route the general kernels take by themselves hangs on the anchor
    in the dead part of the stream (silence: the window's first lag, 200 from cp_start0 and accepted, so the centres leave the tracker within a dozen calls and the
    light walk computes its rows on the spot; noise: anywhere): per stream as PINNED records it, and the same result"""
    c, buf, _ = static
    ncalls = 1100 if call > 250 else 300
    n = ac.nsamples_for(c, ncalls)
    x = buf[:n].copy()
    a = call * L2K + 400
    x[a:] = 0
    if fill == "noise":
        rng = np.random.RandomState(call)
        b = a + 3 * L2K // 2
        x[b:] = (0.05 * (rng.randn(n - b) + 1j * rng.randn(n - b))).astype(np.complex64)
    m = ac.model(c, x, n)
    assert m["status"] == 2 and m["n_symbols"] in (call, call + 1)   # (the window that still sees the partners N earlier may hold a peak of sorts: the model says)
    run_all(c, ac.handle(g, 0), x, n, m, f"lost at {call} {fill}", natural="table")
    if fill == "zeros" and call < 250:                               # the anchor of call 256 sees silence: every lag ties at 0, the first one wins
        got = ac.acquire(g, ac.handle(g, 0), x, n)
        assert got["anchor_pos"][1] == 2111


@pytest.mark.parametrize("call,ncalls", [(243, 250), (244, 250), (245, 250), (1022, 1024), (1023, 1024)])
def test_lost_lock_on_the_placement(static, call, ncalls):
    """the same with no anchor in the dead part of the stream (the calls end in front of the next one): the placement stands, acq_finalize_kernel counts the symbols
    and acq_lost_avg_body leaves the average -- around the 244 calls a workgroup of the placement owns and up to the 1024 of the bookkeeping (a period of 1,025
    calls or more has an anchor at call 1,024, in the silence: test_lost_lock has that one, on the light walk)"""
    c, buf, _ = static
    n = ac.nsamples_for(c, ncalls)
    x = buf[:n].copy()
    x[call * L2K + 400:] = 0
    m = ac.model(c, x, n)
    assert m["status"] == 2 and m["n_symbols"] in (call, call + 1)
    run_all(c, ac.handle(g, 0), x, n, m, f"placement lost at {call}", natural=None)



# ------------------------------------------------------------------------------------------------ acq_small_kernel's verdict on the drift model
@pytest.mark.parametrize("cfo,snr,off", [(0.31, 40.0, 0), (-0.31, 40.0, 0), (0.0, 15.0, 1), (0.0, None, 1), (0.00002, None, 1)])
def test_drift_known_off(po, cfo, snr, off):
    """increments of one sign: the model applies; of both signs (noise around no offset), zero or below DRIFT_MIN_INC: drift_known_off"""
    c, x = ac.symbols(po, 40)
    buf = np.concatenate([np.zeros(300, np.complex64), x])
    if cfo or snr is not None:
        buf = po.channel(buf, c.N, cfo=cfo, snr_db=snr, seed=6, ref_span=(1000, 60000))
    n = ac.nsamples_for(c, 30)
    m = ac.model(c, buf, n)
    assert m["status"] == 0 and m["n_symbols"] == 30
    got = ac.acquire(g, ac.handle(g, 0), buf, n, path=1)
    ac.check(c, m, got, "small", f"cfo {cfo}")
    inc = got["meta"]["incB"][:30]
    min_inc = 2.0 * 2.384185791015625e-07
    one_sign = ((inc > 0).all() or (inc < 0).all()) and (np.abs(inc) >= min_inc).all()
    assert one_sign == (off == 0)
    assert got["rep"].drift_known_off == off


# ------------------------------------------------------------------------------------------------ refusals, buffer discipline
def test_refusals_and_a_second_call(static):
    c, buf, m1100 = static
    rx = ac.handle(g, 0)
    n = ac.nsamples_for(c, 30)
    for kw in ({"hist": -1}, {"hist": (1 << 20) + 1}, {"avail": 0}, {"avail": n + 1}, {"init_tries": 0}, {"init_tries": 65}, {"path": 2}, {"path": -1}, {"force": 3},
               {"force": -1}, {"path": 1, "force": 1}, {"carry": float("nan")}, {"carry": float("inf")}, {"nread": -1}, {"nread": 1 << 20}):
        a = {"hist": 0, "nread": 8}
        a.update(kw)
        assert ac.acquire(g, rx, buf, n, expect=-1, **a) == -1, kw
    assert ac.acquire(g, rx, buf, 2 * c.N + c.cp + 15, expect=-1, nread=1) == -1               # shorter than one window
    assert ac.acquire(g, rx, buf, ac.nsamples_for(c, 769), expect=-1, path=1, nread=8) == -1   # more than ACQ_SMALL_MAX_CALLS calls
    big = np.zeros(ac.nsamples_for(c, 1201), np.complex64)
    assert ac.acquire(g, rx, big, len(big), expect=-1, nread=8) == -1                           # more calls than the handle holds
    # a lost-lock call, then the clean stream on the same handle: the fresh result
    x = buf[:n].copy()
    x[5 * L2K + 400:] = 0
    m = ac.model(c, x, n)
    for route in ("general", "small"):
        ac.run(g, c, rx, x, n, m, route, "lost")
        ac.run(g, c, rx, buf, n, ac.truncate(m1100, c, 30), route, "fresh")
