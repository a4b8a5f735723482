"""symbol8k_kernel and symbol2k_kernel ALONE (dvbt_debug_symbols: a test hook of the library that runs the segment path's own symbol launch), where the chain tests reach
them only behind the acquisition of a synthetic stream: samples and per-symbol metadata built on the host (tests/symcases.py), every tap and output against a float64
demodulator (tests/symref.py, itself checked by tests/test_symref.py).

Bounds: the project's ceilings (ACQ 1e-6 and FFT 1e-5 of the peak, EQ 1e-3 of the spacing) and, tighter, symcases.bounds: 8 times the error of the same statements in
plain float32, per mode, never measured on the kernel.  Labels: exactly the reference's rule (o_demap) on the kernel's own EQ tap, and decide64's wherever the float64
reference lies farther from every decision boundary than the EQ bound.  No launch takes a second of GPU time; nothing here provokes a fault (zeros, NaNs and range-checked
reads are ordinary arithmetic)."""
import ctypes as C

import numpy as np
import pytest

import symcases
import symref

pytestmark = pytest.mark.gpu

MODES = [symcases.T2k, symcases.T8k]
CALLS = 24                                   # what every handle here holds (at most 18 symbols are launched)
FILL = 0x3C                                  # the caller's arrays before a call
A5 = 0xA5                                    # the device buffers before a launch
OUTS = (("labels", np.uint8), ("fo", np.int32), ("mod", np.int32), ("tps", np.complex64), ("acq", np.complex64), ("fft", np.complex64), ("eq", np.complex64),
        ("csi", np.float32))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    L = gr_dvbt_amd.lib()
    L.dvbt_debug_symbols.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + \
        [C.c_void_p] * 8
    return gr_dvbt_amd


@pytest.fixture(scope="module")
def handles(g):
    """one handle per (mode, constellation, hierarchy, guard, soft) setting actually used, taps enabled"""
    made = {}

    def get(setting, soft=0):
        key = tuple(setting) + (soft,)
        if key not in made:
            mode, const, hier, guard = setting
            d = g.get_dims(const, g.C1_2, mode, guard, hier)
            n = 2 * d.fft_length + d.cp_length + 16 + (CALLS - 1) * (d.fft_length + d.cp_length)
            made[key] = g.Rx(const, g.C1_2, mode, max_samples=n, guard=guard, hierarchy=hier, taps=True, soft_decision=soft)
        return made[key]
    yield get
    for rx in made.values():
        rx.close()


def _arrays(T, nread, n_tps):
    shape = {"labels": (nread, T.payload), "fo": (nread,), "mod": (nread,), "tps": (nread, n_tps), "acq": (nread, T.N), "fft": (nread, T.N), "eq": (nread, T.payload),
             "csi": (nread, T.payload)}
    out = {}
    for k, dt in OUTS:
        a = np.empty(shape[k], dt)
        a.view(np.uint8)[...] = FILL
        out[k] = a
    return out


def _call(g, rx, case, nsym=None, keep_last=1, grid=0, delta=None, nread=0, **over):
    """dvbt_debug_symbols on a launch of symcases (arguments replaced by `over`); returns (return code, the output arrays)"""
    T = case.T
    nsym = case.nsym if nsym is None else nsym
    a = {"iq": case.iq, "nsamples": len(case.iq), "call0": case.call0, "avail": case.avail, "cp_start": case.cp_start, "sw": case.sw, "ph_base": case.ph_base,
         "incA": case.incA, "incB": case.incB}
    a.update(over)
    out = _arrays(T, nread or max(nsym, 1), len(T.tps))
    dl = None if delta is None else np.ascontiguousarray(delta, np.float32)
    r = g.lib().dvbt_debug_symbols(rx.h if rx is not None else None, _p(a["iq"]), a["nsamples"], nsym, a["call0"], keep_last, a["avail"], _p(a["cp_start"]), _p(a["sw"]),
                                   _p(a["ph_base"]), _p(a["incA"]), _p(a["incB"]), grid, _p(dl), nread, *[_p(out[k]) for k, _ in OUTS])
    return r, out


def _run(g, rx, case, **kw):
    r, out = _call(g, rx, case, **kw)
    g.binding._chk(r)
    return out


def _is(a, byte):
    return bool((np.ascontiguousarray(a).view(np.uint8) == byte).all())


def _same(a, b, keys=("labels", "fo", "mod", "tps", "acq", "fft", "eq", "csi"), rows=slice(None)):
    """bit-identical (NaNs included)"""
    return [k for k in keys if not np.array_equal(np.ascontiguousarray(a[k][rows]).view(np.uint8), np.ascontiguousarray(b[k][rows]).view(np.uint8))]


RATIOS = {}


def _note(mode, tap, err, po):
    """err / the plain float32 evaluation's error for the tap (what DESIGN.md section 7 quotes), printed with -s"""
    q = err / symcases.float32_errors(po, mode)[tap]
    if q > RATIOS.get((mode, tap), 0.0):
        RATIOS[(mode, tap)] = q
        print(f"RATIO mode {mode} {tap} {q:.3f} (bound at {symcases.FACTOR:.0f})")


def _check(po, mode, case, out, rows=None, labels=True, soft=False, ref=None, taps=("acq", "fft", "eq", "tps"), eq_mask=None, front_rows=None):
    """rows of a launch's outputs against the float64 reference: offsets and patterns equal, the float taps within the working bounds, labels both ways"""
    T, b = case.T, symcases.bounds(po, mode)
    r = case.ref() if ref is None else ref
    rows = list(range(case.nsym)) if rows is None else list(rows)
    front_rows = rows if front_rows is None else list(front_rows)
    assert list(out["fo"][rows]) == list(r["fo"][rows]) and list(out["mod"][rows]) == list(r["mod"][rows]), (out["fo"], out["mod"])
    for k in ("acq", "fft"):
        if k in taps and front_rows:
            peak = np.abs(r[k]).max()
            err = symref.worst(out[k][front_rows], r[k][front_rows]) / peak
            _note(mode, k, err, po)
            assert err <= b[k] <= symcases.CEIL[k], (k, err, b[k])
    for k in ("eq", "tps"):
        if k in taps and rows:
            got, want = out[k][rows], r[k][rows]
            if eq_mask is not None and k == "eq":
                got, want = got[eq_mask[rows]], want[eq_mask[rows]]
            assert np.isfinite(got[np.isfinite(want)]).all(), k
            err = symref.worst(got, want) / T.spacing
            _note(mode, k, err, po)
            assert err <= b[k] <= symcases.CEIL["eq"], (k, err, b[k])
    if soft and rows:
        ok = np.isfinite(r["csi"][rows]) & (r["csi"][rows] > 0)
        err = float(np.abs(out["csi"][rows][ok].astype(np.float64) / r["csi"][rows][ok] - 1).max())
        _note(mode, "csi", err, po)
        assert err <= b["csi"], (err, b["csi"])
    if rows:
        assert (out["labels"][rows] == symref.demap_rule(po, T, out["eq"][rows])).all()            # the reference's rule on the kernel's own values: exact
    if labels and rows:
        want, dist = symref.decide64(T, r["eq"][rows])
        clear = (dist > b["eq"]).all(axis=-1)
        assert 1.0 - clear.mean() <= symcases.SHARE_CAP
        assert (out["labels"][rows][clear] == want[clear]).all()


# ---------------------------------------------------------------- 1, 2: every tap and output; the production instantiation
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chan", ["flat", "echo"])
@pytest.mark.parametrize("const", [0, 1, 2])
def test_every_tap_and_output_and_the_production_instantiation(po, g, handles, mode, const, chan):
    """frame symbols 0..7 and 64..67, carrier shifts -8, -3, 0, +7 from symbol to symbol, a nonzero entry phase and a carrier-offset-sized increment: ACQ, FFT, EQ, TPS
    values, offsets, patterns and labels against the reference.  Then the taps are switched off: the other instantiation gives the same labels, offsets, patterns and TPS
    values bit for bit and hands no tap back (a handle without taps has no tap buffers: the hook leaves the caller's arrays as they were)"""
    name = f"taps_{const}_{chan}"
    case = symcases.case(po, mode, name)
    rx = handles(symcases.setting(mode, name))
    out = _run(g, rx, case)
    _check(po, mode, case, out)
    g.binding._chk(rx.L.dvbt_rx_enable_taps(rx.h, 0))
    try:
        bare = _run(g, rx, case)
    finally:
        g.binding._chk(rx.L.dvbt_rx_enable_taps(rx.h, 1))
    assert not _same(out, bare, ("labels", "fo", "mod", "tps"))
    assert all(_is(bare[k], FILL) for k in ("acq", "fft", "eq", "csi"))
    again = _run(g, rx, case)
    assert not _same(out, again, ("labels", "fo", "mod", "tps", "acq", "fft", "eq"))


@pytest.mark.parametrize("mode", MODES)
def test_soft_decision_handle_delivers_the_channel_state(po, g, handles, mode):
    """a soft_decision = 1 handle: the same instantiation also writes CSI = 1 / |gain|^2, relative error within 8 times the float32 evaluation's"""
    case = symcases.case(po, mode, "taps_1_echo")
    rx = handles(symcases.setting(mode, "taps_1_echo"), soft=1)
    out = _run(g, rx, case)
    _check(po, mode, case, out, soft=True)
    plain = _run(g, handles(symcases.setting(mode, "taps_1_echo")), case)
    assert not _same(out, plain, ("labels", "fo", "mod", "tps", "acq", "fft", "eq"))


# ---------------------------------------------------------------- 3: who takes which symbol
def _jumps_grid1(po, g, handles, mode):
    case = symcases.case(po, mode, "jumps")
    return case, _run(g, handles(symcases.setting(mode, "jumps")), case, grid=1)


@pytest.mark.parametrize("mode", MODES)
def test_result_does_not_depend_on_who_takes_which_symbol(po, g, handles, mode):
    """frame symbols with pattern jumps: the prediction pred = cur_mod + (s - s_prev) of a workgroup is wrong at places that depend on the grid (with one workgroup: at
    every jump; with more: wherever its stride does not match); every output is bit-identical to one workgroup's, which is the reference's"""
    case, one = _jumps_grid1(po, g, handles, mode)
    assert list(case.ref()["mod"]) == [f % 4 for f in symcases.JUMPS]
    _check(po, mode, case, one)
    rx = handles(symcases.setting(mode, "jumps"))
    for grid in (2, 3, 5, case.nsym, 0):
        assert not _same(one, _run(g, rx, case, grid=grid)), grid


# ---------------------------------------------------------------- 4: counts and the last item
@pytest.mark.parametrize("mode", MODES)
def test_counts_and_the_last_item(po, g, handles, mode):
    """nsym from 1 up (2k: groups with inactive quarters), keep_last 0 and 1, on a soft-decision handle (every buffer exists): with keep_last = 0 the last symbol's labels,
    offset / pattern, TPS values, EQ and CSI slots keep their 0xA5, with keep_last = 1 they are the reference's; nothing is written behind symbol nsym - 1"""
    case = symcases.case(po, mode, "counts")
    rx = handles(symcases.setting(mode, "counts"), soft=1)
    for nsym in ((1, 2, 3, 4, 5, 7, 8, 9) if mode == symcases.T2k else (1, 2, 3)):
        for keep in (0, 1):
            out = _run(g, rx, case, nsym=nsym, keep_last=keep, nread=nsym + 3)
            done = nsym if keep else nsym - 1
            _check(po, mode, case, out, rows=range(done), soft=True, front_rows=range(nsym))
            for k, _ in OUTS:
                first = nsym if k in ("acq", "fft") else done                    # (the last item's samples and spectrum are taps of A1 and A2, which have run)
                assert _is(out[k][first:], A5), (nsym, keep, k)


# ---------------------------------------------------------------- 5: the increment switch
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["switch_up", "switch_down"])
def test_increment_switch_at_every_position(po, g, handles, mode, name):
    """incA != incB, of both signs, one symbol per switch position: before, at and behind the first sample, around a 32-sample block, around the thread count, mid-window,
    the window's last samples, the first positions outside [0, N + cp), 2^30.  ACQ and FFT against derotate64: one sample derotated with the wrong increment is off by
    |incA - incB| of its magnitude, a thousand times the bound"""
    case = symcases.case(po, mode, name)
    assert list(case.sw) == symcases.sw_values(mode, case.T.N, case.T.cp)
    out = _run(g, handles(symcases.setting(mode, name)), case)
    _check(po, mode, case, out, labels=False)


# ---------------------------------------------------------------- 6: where the window starts
@pytest.mark.parametrize("mode,guard", [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 3)])
def test_where_the_window_starts(po, g, handles, mode, guard):
    """windows that begin 0, 1, cp / 2 and cp - 1 samples inside the guard interval, mixed from symbol to symbol, for call0 = 3 and, on the same samples less their
    first three symbols, call0 = 0: the window's first sample is (call0 + s)(N + cp) + cp_start - N + 1 and nothing else"""
    name = f"window_g{guard}"
    case = symcases.case(po, mode, name)
    rx = handles(symcases.setting(mode, name))
    out3 = _run(g, rx, case)
    _check(po, mode, case, out3)
    out0 = _run(g, rx, case.moved(0))
    assert not _same(out3, out0)


# ---------------------------------------------------------------- 7: the end of the memory
@pytest.mark.parametrize("mode", MODES)
def test_end_of_the_memory_and_a_symbol_of_zeros(po, g, handles, mode):
    """avail one sample inside, half way through and in front of the last three windows (the range check's zeros; the reference zero-fills), a symbol of zeros in the
    middle.  ACQ and FFT of every symbol within bound; the empty symbols give offset 0 and pattern 0; the cut ones the reference's; EQ within bound wherever the
    reference is finite and the float32 evaluation itself is as accurate as in the other launches (a symbol cut in half has pilots near zero); every label is the
    reference's rule on the kernel's own EQ values, non-finite ones included; the untouched symbols equal those of the launch without the cuts bit for bit"""
    case = symcases.case(po, mode, "edge")
    base, one = _jumps_grid1(po, g, handles, mode)
    out = _run(g, handles(symcases.setting(mode, "edge")), case, grid=1)
    r, r32 = case.ref(), case.ref(np.float32)
    empty = [symcases.EDGE_ZERO, symcases.EDGE_CUT[2]]
    assert all(int(out["fo"][s]) == 0 and int(out["mod"][s]) == 0 for s in empty)
    d = r32["eq"].astype(np.complex128) - r["eq"]
    with np.errstate(all="ignore"):
        mask = np.isfinite(r["eq"]) & (np.maximum(np.abs(d.real), np.abs(d.imag)) <= symcases.float32_errors(po, mode)["eq"] * case.T.spacing)
    assert mask[symcases.EDGE_CUT[0]].mean() > 0.99 and mask[symcases.EDGE_CUT[1]].mean() > 0.5 and not mask[empty].any()
    _check(po, mode, case, out, labels=False, taps=("acq", "fft", "eq"), eq_mask=mask)
    assert not np.abs(out["acq"][empty]).any() and not np.abs(out["acq"][symcases.EDGE_CUT[1]][case.T.N // 2:]).any()
    untouched = [s for s in range(case.nsym) if s != symcases.EDGE_ZERO and s not in symcases.EDGE_CUT]
    assert not _same(one, out, rows=untouched)


# ---------------------------------------------------------------- 8: the DRIFT instantiation
@pytest.mark.parametrize("mode", MODES)
def test_drift_instantiation(po, g, handles, mode):
    """a seeded deviation table within +-1.9e-3: ACQ, FFT and EQ are the reference's with the same table and NOT the reference's without it (so the instantiation ran);
    with the taps off the outputs are the same bit for bit; a following call without a table equals the plain result (the flag word is not left behind)"""
    case = symcases.case(po, mode, "drift")
    rx = handles(symcases.setting(mode, "drift"))
    b = symcases.bounds(po, mode)
    plain = _run(g, rx, case)
    out = _run(g, rx, case, delta=case.delta)
    _check(po, mode, case, out)
    r0 = case.ref(np.float64, delta="none")
    for k, unit in (("acq", np.abs(r0["acq"]).max()), ("fft", np.abs(r0["fft"]).max()), ("eq", case.T.spacing)):
        assert symref.worst(out[k], r0[k]) / unit > 10 * b[k], k
        assert symref.worst(plain[k], r0[k]) / unit <= b[k], k
    g.binding._chk(rx.L.dvbt_rx_enable_taps(rx.h, 0))
    try:
        bare = _run(g, rx, case, delta=case.delta)
    finally:
        g.binding._chk(rx.L.dvbt_rx_enable_taps(rx.h, 1))
    assert not _same(out, bare, ("labels", "fo", "mod", "tps"))
    assert not _same(plain, _run(g, rx, case))


# ---------------------------------------------------------------- 9: hierarchical grids
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["hier_16_a2", "hier_64_a4"])
def test_hierarchical_grids(po, g, handles, mode, name):
    """alpha = 2 and alpha = 4: every carrier takes the candidate search on the shifted grid"""
    case = symcases.case(po, mode, name)
    out = _run(g, handles(symcases.setting(mode, name)), case)
    _check(po, mode, case, out)


# ---------------------------------------------------------------- 10: carriers at the demapper's seams
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("const", [0, 1, 2])
def test_carriers_at_the_demappers_seams(po, g, handles, mode, const):
    """a flat channel, payload carriers on a decision boundary +- 0, 1e-6, 1e-5, 3e-5 and 1e-4 cells (the cell test's margin of 2e-5, the four-candidate search's tie
    rule) and 3.9, 4.1 and 50 cells outside the grid (the exhaustive search): labels are the reference's rule on the kernel's own EQ values, exactly"""
    name = f"seams_{const}"
    case = symcases.case(po, mode, name)
    out = _run(g, handles(symcases.setting(mode, name)), case)
    r = case.ref()
    assert list(out["fo"]) == [0, 0, 0] and list(out["mod"]) == [0, 0, 0]
    _, dist = symref.decide64(case.T, out["eq"])
    assert (dist.min(axis=-1) < 2e-5).sum() > 300 and (dist.min(axis=-1) < 1e-6).sum() > 30        # the seams are where the builder put them, on the kernel's own values
    assert (np.abs(out["eq"]).max(axis=-1) > 40 * case.T.spacing).all()
    assert (out["labels"] == symref.demap_rule(po, case.T, out["eq"])).all()
    assert symref.worst(out["fft"], r["fft"]) <= symcases.CEIL["fft"] * np.abs(r["fft"]).max()


# ---------------------------------------------------------------- 11: refusals
@pytest.mark.parametrize("mode", MODES)
def test_refusals_leave_everything_as_it_was(po, g, handles, mode):
    case = symcases.case(po, mode, "taps_1_flat")
    rx = handles(symcases.setting(mode, "taps_1_flat"))
    T = case.T
    good = _run(g, rx, case)
    n = case.nsym

    def arr(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    before0 = arr(case.cp_start, 0, T.N - 2 - case.call0 * (T.N + T.cp))                               # the window would begin at sample -1
    big = np.zeros((n, T.N // 32), np.float32)
    big[n - 1, -1] = 2e-3
    bad = [dict(iq=None), dict(cp_start=None), dict(sw=None), dict(ph_base=None), dict(incA=None), dict(incB=None),
           dict(nsym=0), dict(nsym=-1), dict(nsym=CALLS + 1), dict(grid=-1), dict(grid=100000), dict(avail=0), dict(avail=-5), dict(avail=len(case.iq) + 1),
           dict(ph_base=arr(case.ph_base, 3, np.nan)), dict(incA=arr(case.incA, 0, np.inf)), dict(incB=arr(case.incB, n - 1, -np.inf)),
           dict(cp_start=before0), dict(delta=big), dict(delta=-big), dict(delta=big * np.nan), dict(nread=n - 1), dict(nread=CALLS + 1)]
    for kw in bad:
        r, out = _call(g, rx, case, **kw)
        assert r == -1, kw
        assert all(_is(out[k], FILL) for k, _ in OUTS), kw
    r, out = _call(g, None, case)
    assert r == -1
    ok = arr(case.cp_start, 0, T.N - 1 - case.call0 * (T.N + T.cp))                                    # ... at sample 0: the first one allowed
    g.binding._chk(_call(g, rx, case, cp_start=ok, nsym=1)[0])
    assert not _same(good, _run(g, rx, case))
