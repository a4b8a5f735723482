"""The channel sounder's model (tests/sounderref.py, the float64 form of the specification in include/dvbt_hip.h) on channels whose answer is known: synthetic
rows Y = H pilots, and the oracle receiver's taps behind pyoracle.channel.  The kernels are held to this model by tests/test_gpu_sounder_block.py; here the
model itself is held to the truth, each of its two corrections is shown to be needed, and the host helpers of gr_dvbt_amd.SounderReading are held to the
model's.  No GPU."""
import numpy as np
import pytest

import sounderref as sr


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert hasattr(gr_dvbt_amd, "Sounder") and hasattr(gr_dvbt_amd, "SounderReading")
    return gr_dvbt_amd


def _level(reading, delay):
    """the five-bin level in dB, relative to the strongest, of the path found within a sample of `delay`"""
    hits = [lev for d, lev in reading.paths(-60.0) if abs(d - delay) <= 1.0]
    assert hits, (delay, reading.paths(-40.0))
    return max(hits)


def _elsewhere_db(reading, delays, keep=4):
    """the largest bin outside +-keep bins of the known paths (0 is one), in dB relative to the strongest bin"""
    p, m0 = reading.pdp, int(np.argmax(reading.pdp))
    mask = np.ones(reading.M, bool)
    for d in (0,) + tuple(delays):
        centre = m0 + 1.5 * d
        for m in range(int(np.floor(centre)) - keep, int(np.ceil(centre)) + keep + 1):
            mask[m % reading.M] = False
    return 10.0 * np.log10(p[mask].max() / p[m0])


# ------------------------------------------------------------------ 1. synthetic rows
@pytest.mark.parametrize("mode", [0, 1])
def test_a_unit_path_reads_one(g, mode):
    md = sr.Mode(mode)
    rows = sr.pilot_rows(md, range(8, 16), rng=np.random.RandomState(mode))
    for window in (sr.RECT, sr.HANN):
        r = sr.sound(rows, mode=mode, window=window, first_index=8)
        assert (r.groups_used, r.groups_skipped, r.symbols_pushed) == (2, 0, 8)
        assert abs(r.pdp[0] / r.groups_used - 1.0) <= 1e-4
        assert np.allclose(r.resp / r.groups_used, 1.0, atol=1e-12)
        assert r.ripple_db() < 1e-9
        if window == sr.HANN:                      # (the rectangular window's own side lobes stand at -13 dB)
            assert r.paths() == [(0.0, 0.0)]


@pytest.mark.parametrize("paths", [((20, 0.3),), ((56, 0.2j),), ((56, 0.15), (20, -0.1j)), ((-14, 0.25),), ((300, 0.1 - 0.1j),)], ids=str)
def test_paths_at_even_delays_read_their_levels(g, paths):
    md = sr.Mode(0)
    H = sr.channel_of_paths(md, ((0, 1.0),) + paths)
    rows = sr.pilot_rows(md, range(4, 12), H=H, rng=np.random.RandomState(3), offset=-3)
    r = sr.sound(rows, offset=np.full(8, -3), mode=0, first_index=4)
    assert r.groups_used == 2
    for d, a in paths:
        got, want = _level(r, d), 20.0 * np.log10(abs(a))
        print(f"path {d}: {got:.3f} dB ({want:.3f})")
        assert abs(got - want) <= 0.25
    found = [d for d, _ in r.paths(-30.0)]
    assert len(found) == 1 + len(paths), r.paths(-30.0)


def test_the_helpers_of_the_binding_are_the_models(g):
    md = sr.Mode(0)
    H = sr.channel_of_paths(md, ((0, 1.0), (19, 0.3), (-40, 0.1j), (200, 0.05)))
    want = sr.sound(sr.pilot_rows(md, range(0, 8), H=H), mode=0)
    got = g.SounderReading(want.pdp, want.resp, 8, 2, 0, 0)
    assert np.array_equal(got.delays(), want.delays()) and np.array_equal(got.delays(1e6), want.delays(1e6))
    assert got.paths() == want.paths() and got.paths(-40.0) == want.paths(-40.0) and len(want.paths()) == 4
    assert got.outside_guard_db(64) == want.outside_guard_db(64) and got.ripple_db() == want.ripple_db()
    # the pre-echo and the echo beyond the guard interval: 0.01 + 0.0025 of 1 + 0.09 + 0.01 + 0.0025
    assert abs(want.outside_guard_db(64) - 10.0 * np.log10(0.0125 / 1.1025)) < 0.1
    assert want.delays()[int(np.argmax(want.pdp))] == 0.0 and want.delays().min() == -md.M / 3.0


# ------------------------------------------------------------------ 2. which groups are used
def test_skipping_skips_exactly_the_broken_group(g):
    md = sr.Mode(0)
    rows = sr.pilot_rows(md, range(0, 20))
    base = dict(index=np.arange(20) % 68, offset=np.zeros(20, int), cp_start=np.full(20, 500))
    whole = sr.sound(rows, mode=0, **base)
    assert (whole.groups_used, whole.groups_skipped) == (5, 0)
    for what, key, at, value in (("an index jump inside a group", "index", 9, 10), ("an offset change", "offset", 6, 1), ("delta 65", "cp_start", 14, 565),
                                 ("delta -65", "cp_start", 3, 435), ("an index above 67", "index", 16, 68), ("an offset below -8", "offset", 0, -9)):
        args = {k: v.copy() for k, v in base.items()}
        args[key][at] = value
        if key == "offset" and at % 4 == 0:
            args[key][at:at + 4] = value           # all four equal, and out of range
        r, each = sr.sound(rows, mode=0, per_group=True, **args)
        assert (r.groups_used, r.groups_skipped) == (4, 1), what
        assert [q for q, _ in each] == [q for q in range(5) if q != at // 4], what
        assert abs(r.pdp[0] - 4.0) < 1e-3, what
    args = {k: v.copy() for k, v in base.items()}
    args["cp_start"][12:16] += np.array([0, 64, -64, 1])
    assert sr.sound(rows, mode=0, **args).groups_skipped == 0                     # |delta| = 64 is still used
    assert sr.sound(rows[:19], mode=0).groups_used == 4                           # an open group adds nothing
    assert sr.sound(rows, mode=0, index=(np.arange(20) + 66) % 68).groups_used == 5   # 66, 67, 0, 1 are consecutive


# ------------------------------------------------------------------ 3. the oracle receiver's taps
CHANNELS = {
    "none": dict(),
    "echo (19, 0.3)": dict(echoes=((19, 0.3),)),
    "echo (57, 0.2j)": dict(echoes=((57, 0.2j),)),
    "echoes (57, 0.15), (19, -0.1j), cfo 3.37": dict(echoes=((57, 0.15), (19, -0.1j)), cfo=3.37),
    "echo (19, 0.3), cfo -2.37, 25 dB AWGN": dict(echoes=((19, 0.3),), cfo=-2.37, snr_db=25.0),
}
_taps = {}


def oracle_taps(po, name):
    """(rows, index, offset, cp_start) from symbol 8 on of one superframe of 2k QAM16 1/2, seed 9, through the channel: computed once"""
    if name not in _taps:
        c = po.cfg(1, 0, 0)
        iq = po.channel(po.stream_slice(c, 1, 9), c.N, **CHANNELS[name])
        o = po.rx(c, iq, want=("fft",))
        n = len(o["fft"]) - 1
        assert n >= 268 and len(o["lock_periods"]) == 1, "the case is meant to hold the lock"
        _taps[name] = tuple(np.array(a[8:n]) for a in (o["fft"], o["sym_index"], o["freq_offset"], o["cp_start"]))
        for a in _taps[name]:
            a.setflags(write=False)
    return _taps[name]


@pytest.mark.parametrize("name", list(CHANNELS))
def test_the_oracles_taps_read_the_channel_that_was_set(g, po, name):
    rows, idx, off, cps = oracle_taps(po, name)
    r = sr.sound(rows, idx, off, cps, mode=0)
    echoes = CHANNELS[name].get("echoes", ())
    assert r.groups_skipped == 0 and r.groups_used == len(rows) // 4 >= 65
    for d, a in echoes:
        got, want = _level(r, d), 20.0 * np.log10(abs(a))
        print(f"[{name}] echo at {d}: {got:.3f} dB ({want:.3f})")
        assert abs(got - want) <= 0.25
    elsewhere = _elsewhere_db(r, [d for d, _ in echoes])
    print(f"[{name}] largest elsewhere {elsewhere:.1f} dB, median bin {10 * np.log10(np.median(r.pdp) / r.pdp.max()):.1f} dB")
    assert elsewhere <= -35.0
    assert [round(d) for d, _ in r.paths()] == sorted([0] + [d for d, _ in echoes])


def _quarter_span_image_db(reading, keep=4):
    """the largest bin within +-keep of a quarter, a half or three quarters of the span behind the strongest, in dB relative to it"""
    p, m0, M = reading.pdp, int(np.argmax(reading.pdp)), reading.M
    return max(10.0 * np.log10(p[(m0 + q * M // 4 + np.arange(-keep, keep + 1)) % M].max() / p[m0]) for q in (1, 2, 3))


def test_the_common_phase_alignment_is_needed(g, po):
    rows, idx, off, cps = oracle_taps(po, "echoes (57, 0.15), (19, -0.1j), cfo 3.37")
    without, with_ = sr.sound(rows, idx, off, cps, mode=0, phase=False), sr.sound(rows, idx, off, cps, mode=0)
    print(f"image without r_i {_quarter_span_image_db(without):.1f} dB, with {_quarter_span_image_db(with_):.1f} dB")
    assert _quarter_span_image_db(without) > -10.0 and _quarter_span_image_db(with_) < -35.0


def test_the_timing_correction_is_needed(g, po):
    rows, idx, off, cps = oracle_taps(po, "echo (19, 0.3)")
    assert len(set(cps.tolist())) > 1, "the tracker moves cp_start"
    without, with_ = sr.sound(rows, idx, off, cps, mode=0, timing=False), sr.sound(rows, idx, off, cps, mode=0)
    print(f"image without tau {_quarter_span_image_db(without):.1f} dB, with {_quarter_span_image_db(with_):.1f} dB")
    assert _quarter_span_image_db(without) > -25.0 and _quarter_span_image_db(with_) < -35.0
