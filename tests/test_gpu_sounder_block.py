"""The GPU channel sounder (dvbt_sounder_*, gr_dvbt_amd.Sounder) against its float64 model tests/sounderref.py.

The per-bin bound has the form of the spectrum analyser's: test_gpu_fft_sizes holds a transform's amplitudes to 1e-5 of its peak, so a bin's power is off by at
most 2e-5 sqrt(P Pmax) (Pmax: the largest bin of the profile, P and Pmax both sums over the same groups), plus 1e-10 Pmax where P is next to nothing, plus
1e-6 P for r_i's normalisation and the float sums of a run of 8 groups.  resp, which no transform touches, is held to 2e-6 of itself.  The counts are
integers and compared exactly.  What a stream looks like cut into calls, through the host or the device entry, after a reset or on two streams is compared bit
for bit: the doubles of pdp and resp, every count.
"""
import ctypes as C

import numpy as np
import pytest

import sounderref as sr

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

R = sr.RUN
COUNTS_2K = (0, 1, 3, 4, 5, 7, 8, 9, 4 * R - 1, 4 * R, 4 * R + 1, 8 * R + 4)
WINDOWS = {sr.RECT: "rect", sr.HANN: "hann"}


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    L = gr_dvbt_amd.lib()
    L.dvbt_device_malloc.restype = C.c_void_p
    L.dvbt_device_malloc.argtypes = [C.c_size_t]
    L.dvbt_device_free.argtypes = [C.c_void_p]
    L.dvbt_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    assert gr_dvbt_amd.Sounder is not None
    return gr_dvbt_amd


class Dev:
    """an array on the device (the library's own allocator and blocking copies: ordered with work on the default stream)"""

    def __init__(self, g, x):
        self.L = g.lib()
        x = np.ascontiguousarray(x)
        self.itemsize = x.dtype.itemsize * (x.shape[1] if x.ndim == 2 else 1)
        self.base = self.L.dvbt_device_malloc(x.nbytes + 64)
        assert self.base and self.base % 16 == 0
        if x.nbytes:
            assert self.L.dvbt_copy_to_device(C.c_void_p(self.base), x.ctypes.data_as(C.c_void_p), x.nbytes) == 0

    def at(self, row):
        return self.base + self.itemsize * row

    def free(self):
        self.L.dvbt_device_free(C.c_void_p(self.base))


def _bits(r):
    return (r.pdp.tobytes(), r.resp.tobytes(), r.symbols_pushed, r.groups_used, r.groups_skipped)


_streams = {}


def stream(mode, n, offset=0, seed=1):
    """n rows behind a three-path channel, with QAM16 on the data carriers, complex64; indices from 5 on, cp_start moving by -2 .. 1 inside the groups.
    Computed once per (mode, n, offset) and left unchanged."""
    key = (mode, n, offset, seed)
    if key not in _streams:
        md = sr.Mode(mode)
        rng = np.random.RandomState(seed + mode)
        idx = (5 + np.arange(n)) % 68
        H = sr.channel_of_paths(md, ((0, 1.0), (19, 0.3), (150, -0.1j), (-30, 0.05)))
        cps = 700 + np.array([(0, -2, 1, 0), (0, 1, 1, -2), (0, 0, 0, 0)])[np.arange(n) // 4 % 3, np.arange(n) % 4]
        rows = sr.pilot_rows(md, idx, H=H, rng=rng, offset=offset)
        # what a receiver whose window moved by delta and whose phase turned sees: the model's corrections then have something to undo
        k = np.arange(md.K) - md.c0
        for s in range(n):
            d = cps[s] - cps[4 * (s // 4)] if 4 * (s // 4) < n else 0
            rows[s, md.zl + offset:md.zl + offset + md.K] *= np.exp(2j * np.pi * k * d / md.N) * np.exp(1j * rng.uniform(-np.pi, np.pi))
        out = (rows.astype(np.complex64), idx.astype(np.int32), np.full(n, offset, np.int32), cps.astype(np.int32))
        for a in out:
            a.setflags(write=False)
        _streams[key] = out
    return _streams[key]


def _check_against_model(got, want, what):
    """the counts exact, pdp within the bound, resp to 2e-6; returns the worst ratio of a pdp bin's error to its bound"""
    assert (got.symbols_pushed, got.groups_used, got.groups_skipped) == (want.symbols_pushed, want.groups_used, want.groups_skipped), what
    if want.groups_used == 0:
        assert not got.pdp.any() and not got.resp.any(), what
        return 0.0
    pmax = want.pdp.max()
    bound = 2e-5 * np.sqrt(want.pdp * pmax) + 1e-10 * pmax + 1e-6 * want.pdp
    ratio = float((np.abs(got.pdp - want.pdp) / bound).max())
    assert ratio <= 1.0, (what, ratio)
    assert np.abs(got.resp - want.resp).max() <= 2e-6 * want.resp.max(), what
    return ratio


# ------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize("offset", [-8, 0, 7])
@pytest.mark.parametrize("kind", sorted(WINDOWS))
def test_2k_profiles_against_the_model(g, kind, offset):
    rows, idx, off, cps = stream(0, max(COUNTS_2K), offset)
    s = g.Sounder(g.T2k, WINDOWS[kind])
    worst = 0.0
    for n in COUNTS_2K:
        s.reset()
        s.push(rows[:n], idx[:n], off[:n], cps[:n])
        want = sr.sound(rows[:n], idx[:n], off[:n], cps[:n], mode=0, window=kind)
        assert want.groups_used == n // 4
        worst = max(worst, _check_against_model(s.read(), want, (kind, offset, n)))
    print(f"\n2k {WINDOWS[kind]} offset {offset}: worst pdp error {worst:.3f} of the bound")
    s.close()


@pytest.mark.parametrize("n", [8, 4 * R + 4])
def test_8k_profiles_against_the_model(g, n):
    rows, idx, off, cps = stream(1, 4 * R + 4, -3)
    worst = 0.0
    for kind in sorted(WINDOWS):
        s = g.Sounder(g.T8k, WINDOWS[kind])
        s.push(rows[:n], idx[:n], off[:n], cps[:n])
        want = sr.sound(rows[:n], idx[:n], off[:n], cps[:n], mode=1, window=kind)
        worst = max(worst, _check_against_model(s.read(), want, (kind, n)))
        s.close()
    print(f"\n8k {n} symbols: worst pdp error {worst:.3f} of the bound")


def test_rows_straight_from_a_modulator_need_no_int_arrays(g):
    md = sr.Mode(0)
    rows = sr.pilot_rows(md, (63 + np.arange(12)) % 68, H=sr.channel_of_paths(md, ((0, 1.0), (40, 0.5))), rng=np.random.RandomState(4)).astype(np.complex64)
    s = g.Sounder(g.T2k, first_index=63)
    s.push(rows)
    want = sr.sound(rows, mode=0, first_index=63)
    assert want.groups_used == 3
    _check_against_model(s.read(), want, "null arrays")
    got = s.read().paths()
    assert len(got) == 2 and got[1][0] == 40.0 and abs(got[1][1] - 20 * np.log10(0.5)) <= 0.25
    s.close()


# ------------------------------------------------------------------ 2. the counts
BREAKS = (("an index jump inside a group", 1, 9, 30), ("an offset change", 2, 6, 1), ("delta 65", 3, 14, 765), ("delta -65", 3, 3, 635),
          ("an index above 67", 1, 16, 68), ("an index below 0", 1, 20, -1), ("an offset above 7", 2, 13, 8), ("an offset far below -8", 2, 24, -100000),
          ("a cp_start at the end of int", 3, 29, 2 ** 31 - 1))


@pytest.mark.parametrize("what,which,at,value", BREAKS, ids=[b[0] for b in BREAKS])
def test_a_broken_group_is_skipped_and_counted(g, what, which, at, value):
    arrays = [a.copy() for a in stream(0, 4 * R + 4)]
    arrays[which][at] = value
    if which == 2 and at % 4 == 0:
        arrays[2][at:at + 4] = value               # the four offsets equal, and out of range
    want = sr.sound(*arrays, mode=0)
    assert (want.groups_used, want.groups_skipped) == (R, 1), what
    for calls in ((4 * R + 4,), (at, 1, 4 * R + 3 - at), (at + 1, 4 * R + 3 - at)):
        s = g.Sounder(g.T2k)
        a = 0
        for n in calls:
            s.push(*[x[a:a + n] for x in arrays])
            a += n
        _check_against_model(s.read(), want, (what, calls))
        s.close()


# ------------------------------------------------------------------ 3. a stream cut into calls
def _cuts(n, pattern):
    out, a, i = [], 0, 0
    while a < n:
        out.append(min(pattern[i % len(pattern)], n - a))
        a += out[-1]
        i += 1
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_a_stream_cut_into_calls_gives_the_bits_of_one_call(g, mode):
    n = 8 * R + 7 if mode == 0 else 4 * R + 7
    arrays = stream(mode, n, 2)
    dev = [Dev(g, a) for a in arrays]
    s = g.Sounder(mode)
    s.push(*arrays)
    one = s.read()
    assert one.groups_used == n // 4 and one.pdp.max() > 0
    for pattern in ((n,), (1,), (3, 5, 1, 0, 7, 2, 4, 6)):
        for entry in ("host", "device"):
            if mode == 1 and pattern == (1,) and entry == "host":
                continue                           # (the 2k run covers one symbol per host call)
            s.reset()
            a = 0
            for c in _cuts(n, pattern) + [0]:
                if entry == "host":
                    s.push(*[x[a:a + c] for x in arrays])
                else:
                    s.push_device(dev[0].at(a), c, dev[1].at(a), dev[2].at(a), dev[3].at(a))
                a += c
            assert _bits(s.read()) == _bits(one), (pattern, entry)
            assert _bits(s.read()) == _bits(one), "a read does not disturb the accumulation"
    # a read between the calls changes nothing either
    s.reset()
    s.push(*[x[:13] for x in arrays])
    part = s.read()
    assert (part.symbols_pushed, part.groups_used) == (13, 3)
    s.push(*[x[13:] for x in arrays])
    assert _bits(s.read()) == _bits(one)
    s.close()
    for d in dev:
        d.free()


def test_a_refused_call_leaves_the_stream_where_it_was(g):
    arrays = stream(0, 4 * R + 4)
    s = g.Sounder(g.T2k)
    s.push(*[x[:6] for x in arrays])
    L, PI = g.lib(), C.POINTER(C.c_int)
    rows = np.zeros((3, 2048), np.complex64)
    ptr = rows.ctypes.data
    ints = np.zeros(8, np.int32)
    refusals = (
        ("null rows", None, None, 2),
        ("misaligned rows", C.c_void_p(ptr + 4), None, 2),
        ("a misaligned int array", C.c_void_p(ptr), C.cast(C.c_void_p(ints.ctypes.data + 2), PI), 2),
        ("more than 2^24 symbols", C.c_void_p(ptr), None, (1 << 24) + 1),
    )
    for what, r, i, n in refusals:
        assert L.dvbt_sounder_push(s.h, r, i, None, None, n) == -1, what
        assert L.dvbt_sounder_push_device(s.h, r, i, None, None, n, None) == -1, what
    res = g.SounderResult()
    small = np.zeros(8, np.float64)
    assert L.dvbt_sounder_read(s.h, C.byref(res), small.ctypes.data_as(C.POINTER(C.c_double)), 8, None, 0) == -1
    assert L.dvbt_sounder_read(s.h, C.byref(res), None, 0, small.ctypes.data_as(C.POINTER(C.c_double)), 8) == -1
    assert L.dvbt_sounder_read(s.h, C.byref(res), None, 0, None, 0) == 0 and (res.symbols_pushed, res.groups_used, res.M, res.Kp) == (6, 1, 1024, 569)
    s.push(*[x[6:] for x in arrays])
    want = g.Sounder(g.T2k)
    want.push(*arrays)
    assert _bits(s.read()) == _bits(want.read())
    s.close()
    want.close()


# ------------------------------------------------------------------ 4. handles and streams
def test_two_handles_on_two_streams_and_a_change_of_stream(g):
    assert torch is not None
    n = 8 * R + 6
    arrays = stream(0, n, 2)
    other = stream(0, n, -8, seed=7)
    dev, dev2 = [Dev(g, a) for a in arrays], [Dev(g, a) for a in other]
    a, b = g.Sounder(g.T2k), g.Sounder(g.T2k, "rect")
    a.push(*arrays)
    b.push(*other)
    want_a, want_b = _bits(a.read()), _bits(b.read())
    a.reset()
    b.reset()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pos = 0
    for i, c in enumerate(_cuts(n, (5, 9, 2, 16))):
        sa, sb = (s1, s2) if i % 2 == 0 else (s2, s1)              # each handle changes its stream with every call
        a.push_device(dev[0].at(pos), c, dev[1].at(pos), dev[2].at(pos), dev[3].at(pos), stream=sa.cuda_stream)
        b.push_device(dev2[0].at(pos), c, dev2[1].at(pos), dev2[2].at(pos), dev2[3].at(pos), stream=sb.cuda_stream)
        pos += c
    assert _bits(a.read()) == want_a and _bits(b.read()) == want_b
    a.close()
    b.close()
    for d in dev + dev2:
        d.free()


# ------------------------------------------------------------------ 5. end to end on the device
CHANNELS = [("no echo", dict()), ("echo (19, 0.3)", dict(echoes=((19, 0.3),))), ("echo (57, 0.2j)", dict(echoes=((57, 0.2j),))),
            ("echoes (57, 0.15), (19, -0.1j), cfo 3.37", dict(echoes=((57, 0.15), (19, -0.1j)), cfo=3.37))]


@pytest.fixture(scope="module")
def baseband(g):
    """one superframe of 2k QAM16 1/2 from the modulator, behind 1000 zeros and in front of 3 N: the synthetic stream of seed 9 that the model's test
    takes from the oracle (pyoracle.stream_ts and tx_scale, written out here), on which the reference's tracker is known to move cp_start by a sample
    at a time.  (A profile is referred to the cp_start of each group's first symbol: on a transport stream of other bytes the tracker started two groups
    of 65 two samples late, which moved their main lobe by three bins and read -22.2 dB five bins in front of the strongest -- on the device and in the
    model alike.)"""
    scale = float(np.float32(0.0022097087) * np.float32(0.0022097087))
    tx = g.Tx(g.QAM16, g.C1_2, g.T2k, scale=scale)
    d = tx.dims
    npk = 272 * d.payload_length * d.m * d.cr_k // d.cr_n // 8 // 204
    ts = np.random.RandomState(9 * 1000003).randint(0, 256, size=(npk, 188)).astype(np.uint8)
    ts[:, 0] = 0x47
    iq = tx.run(ts)
    tx.close()
    assert len(iq) == 272 * (d.fft_length + d.cp_length)
    out = np.concatenate([np.zeros(1000, np.complex64), iq, np.zeros(3 * 2048, np.complex64)])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name,chan", CHANNELS, ids=[c[0] for c in CHANNELS])
def test_end_to_end_behind_the_channel_block(g, baseband, name, chan):
    echoes = chan.get("echoes", ())
    ch = g.Channel(echoes=echoes, cfo=chan.get("cfo", 0.0), fft_length=2048)
    iq = ch.run(baseband)
    ch.close()
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=len(iq), taps=True)
    rep = rx.run(iq)
    assert rep.n_symbols >= 268, "the case is meant to hold the lock over the whole superframe"
    s = g.Sounder.from_rx(rx, first_row=8)
    got = s.read()
    n = rep.n_symbols - 1
    taps = [np.array(rx.tap(t)[8:n]) for t in (g.TAP_FFT, g.TAP_SYMBOL_INDEX, g.TAP_FREQ_OFFSET, g.TAP_CP_START)]
    want = sr.sound(*taps, mode=0)
    assert want.groups_skipped == 0 and want.groups_used == (n - 8) // 4
    ratio = _check_against_model(got, want, name)
    found = got.paths()
    print(f"\n[{name}] {got.groups_used} groups, worst pdp error {ratio:.3f} of the bound, paths {[(round(d, 2), round(v, 3)) for d, v in found]}")
    assert len(found) == 1 + len(echoes), found
    for d, a in echoes:
        hit = [lev for dd, lev in found if abs(dd - d) <= 1.0]
        assert len(hit) == 1 and abs(hit[0] - 20.0 * np.log10(abs(a))) <= 0.25, (d, found)
    m0, mask = int(np.argmax(got.pdp)), np.ones(got.M, bool)
    for d in (0,) + tuple(d for d, _ in echoes):
        for m in range(int(np.floor(m0 + 1.5 * d)) - 4, int(np.ceil(m0 + 1.5 * d)) + 5):
            mask[m % got.M] = False
    elsewhere = 10.0 * np.log10(got.pdp[mask].max() / got.pdp[m0])
    print(f"[{name}] largest elsewhere {elsewhere:.1f} dB")
    assert elsewhere <= -35.0
    s.close()
    rx.close()
