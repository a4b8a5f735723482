"""The GPU crest-factor reduction block (dvbt_cfr_*, gr_dvbt_amd.Cfr) against its numpy model tests/cfrref.py, on symbols the GPU modulator made.

Shapes: 2k with G = 1/32, 8 symbols, first_symbol 0 and 3 (all four scattered-pilot phases and the wrap); 8k with G = 1/4, 4 symbols (the largest LDS image
and the largest prefix).
TOL: a symbol goes through T = 1 + 2 os iterations transforms; 1e-5 of the peak per transform is the FFT block's own bound (tests/test_gpu_fft_sizes.py), and
clip, mask and phase average are non-expansive, so the errors add at worst linearly: max |out - model| <= T 1e-5 max |model|.
The counters are compared exactly, at a threshold for which the model says that no first-iteration |x_p[n]| lies within 1e-4 A of A (the margin is asserted):
float32 transforms are two orders of magnitude closer than that.  Whatever a stream looks like cut into calls, run in place, on two streams or by two
handles is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import cfrref as cr

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

PAPR_DB = 7.0
SHAPES = {"2k": (0, 0, 8), "8k": (1, 3, 4)}          # transmission mode, guard interval, symbols
CASES = [("2k", 0), ("2k", 3), ("8k", 0)]            # shape, first_symbol
MARGIN = 1e-4


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    L = gr_dvbt_amd.lib()
    L.dvbt_device_malloc.restype = C.c_void_p
    L.dvbt_device_malloc.argtypes = [C.c_size_t]
    L.dvbt_device_free.argtypes = [C.c_void_p]
    L.dvbt_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return gr_dvbt_amd


class Dev:
    """n complex64 on the device (the library's own allocator and blocking copies: ordered with work on the default stream)"""

    def __init__(self, g, x=None, n=None):
        self.L = g.lib()
        self.n = len(x) if x is not None else n
        self.ptr = self.L.dvbt_device_malloc(8 * self.n + 64)
        assert self.ptr and self.ptr % 16 == 0
        self.put(np.zeros(self.n, np.complex64) if x is None else x)

    def put(self, x, at=0):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if len(x):
            assert self.L.dvbt_copy_to_device(C.c_void_p(self.ptr + 8 * at), x.ctypes.data_as(C.c_void_p), 8 * len(x)) == 0

    def get(self, at=0, n=None):
        n = self.n - at if n is None else n
        out = np.zeros(n, np.complex64)
        if n:
            assert self.L.dvbt_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + 8 * at), 8 * n) == 0
        return out

    def free(self):
        self.L.dvbt_device_free(C.c_void_p(self.ptr))
        self.ptr = None


def _tx_symbols(g, mode, guard, nsym, seed):
    """the first nsym symbols of the GPU modulator's output for a random transport stream (QAM64 7/8), made on the device and copied out"""
    md = cr.Mode(mode, guard)
    npk = 64 if mode == 0 else 160
    rng = np.random.RandomState(seed)
    ts = rng.randint(0, 256, (npk, 188)).astype(np.uint8)
    ts[:, 0] = 0x47
    L = g.lib()
    tx = g.Tx(g.QAM64, g.C7_8, (g.T2k, g.T8k)[mode], guard=guard, max_packets=npk)
    cap = tx.samples_for(npk)
    assert cap >= nsym * md.symbol and cap % md.symbol == 0
    dts = L.dvbt_device_malloc(ts.size + 64)
    assert L.dvbt_copy_to_device(C.c_void_p(dts), ts.ctypes.data_as(C.c_void_p), ts.size) == 0
    d = Dev(g, n=cap)
    assert tx.run_device(dts, npk, d.ptr, cap) == cap
    x = d.get(0, nsym * md.symbol)
    tx.close(); d.free(); L.dvbt_device_free(C.c_void_p(dts))
    return md, x


@pytest.fixture(scope="module")
def streams(g):
    """per shape: (mode, guard, the model's Mode, the symbols, their mean power)"""
    out = {}
    for name, (mode, guard, nsym) in SHAPES.items():
        md, x = _tx_symbols(g, mode, guard, nsym, 11 + mode)
        assert np.isfinite(x.view(np.float32)).all()
        out[name] = (mode, guard, md, x, float(np.mean(np.abs(x.astype(np.complex128)) ** 2)))
    return out


def _threshold(md, x, power, os, first=0):
    """a threshold near PAPR_DB over the mean at which the model's first-iteration decisions stand clear of rounding: the first of PAPR_DB + 0.01 i dB,
    i < 16, with a margin above 2 MARGIN.  As the float32 the block is given."""
    for i in range(16):
        A = float(np.float32(cr.threshold_for(PAPR_DB + 0.01 * i, power)))
        ctr = cr.new_counters()
        for l, row in enumerate(x.reshape(-1, md.symbol)):
            cr.run_symbol(md, row, first + l, A, 1, os, 3, ctr)
        if ctr["margin"] > 2 * MARGIN:
            return A
    raise AssertionError("no threshold with a clear margin among the candidates")


def _reading(ctr):
    return tuple(ctr[f] for f in cr.FIELDS[:4])


def _check(g, got, reading, ref, ctr, T, what):
    assert got.shape == ref.shape and got.dtype == np.complex64
    err, peak = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"\n{what}: largest error {err:.3e} = {err / peak:.2e} of the peak (bound {T * 1e-5:.1e}); model margin {ctr['margin']:.2e}; {reading}")
    assert err <= T * 1e-5 * peak
    assert ctr["margin"] > MARGIN, "the model's own decisions must not hang on rounding"
    assert reading.as_tuple()[:4] == _reading(ctr)
    assert abs(reading.peak_power_in - ctr["peak_power_in"]) <= 1e-5 * ctr["peak_power_in"]


# ------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize("iterations", [1, 4])
@pytest.mark.parametrize("os", [1, 2, 4])
@pytest.mark.parametrize("shape,first", CASES, ids=[f"{s}_first{f}" for s, f in CASES])
def test_output_and_counters_against_the_model(g, streams, shape, first, os, iterations):
    mode, guard, md, x, power = streams[shape]
    A = _threshold(md, x, power, os, first)
    ref, ctr = cr.run(md, x, A, iterations, os, first_symbol=first)
    f = g.Cfr(mode, guard, A, iterations, os, first_symbol=first)
    assert f.p.threshold == A
    got = f.run(x)
    reading = f.read()
    assert reading == f.read()                                    # a read repeated
    f.close()
    assert ctr["symbols_clipped"] == ctr["symbols"] == len(x) // md.symbol and ctr["samples_over"] > 0
    _check(g, got, reading, ref, ctr, 1 + 2 * os * iterations, f"{shape} first {first} os {os} it {iterations}")
    rows = got.reshape(-1, md.symbol)
    assert (rows[:, :md.G] == rows[:, md.N:]).all(), "the prefix is the useful part's end, bit for bit"


@pytest.mark.parametrize("keep", [0, cr.KEEP_PILOTS, cr.KEEP_TPS])
def test_keep_masks_against_the_model(g, streams, keep):
    mode, guard, md, x, power = streams["2k"]
    A = _threshold(md, x, power, 2, 1)
    ref, ctr = cr.run(md, x, A, 2, 2, keep, 1)
    f = g.Cfr(mode, guard, A, 2, 2, keep, first_symbol=1)
    got, reading = f.run(x), f.read()
    f.close()
    _check(g, got, reading, ref, ctr, 1 + 2 * 2 * 2, f"keep {keep}")


def test_the_modulators_pilots_and_tps_come_through(g, streams):
    """the block's symbol 0 is the frame's symbol 0 of the modulator: with the default `keep` its pilots and TPS carriers are where they were (to the
    rounding of two transforms), while the data carriers have moved"""
    for shape in SHAPES:
        mode, guard, md, x, power = streams[shape]
        f = g.Cfr(mode, guard, g.Cfr.threshold_for(PAPR_DB, power))
        got = f.run(x)
        f.close()
        X0 = np.fft.fft(x.astype(np.complex128).reshape(-1, md.symbol)[:, md.G:], axis=1)
        X = np.fft.fft(got.astype(np.complex128).reshape(-1, md.symbol)[:, md.G:], axis=1)
        scale = np.abs(X0).max()
        for l in range(len(X)):
            kept = md.bins(md.kept(l, 3))
            d = np.abs(X[l] - X0[l])
            assert d[kept].max() <= 2e-5 * scale and np.median(d[md.free(l, 3)]) > 1e-3 * scale
            sp = X0[l][md.bins(md.scattered(l))]
            assert np.ptp(np.abs(sp)) <= 1e-5 * scale and np.abs(sp.imag).max() <= 1e-5 * scale, "one amplitude, real: these ARE the scattered pilots"
            assert np.ptp(np.abs(X0[l][md.bins(md.scattered(l + 1))])) > 0.1 * scale, "and those of the next symbol are not"
            assert d[~md.occupied].max() <= 2e-5 * scale


# ------------------------------------------------------------------ 2. pass-through
def test_pass_through_is_bitwise(g, streams):
    mode, guard, md, x, power = streams["2k"]
    A = _threshold(md, x, power, 2)
    # iterations = 0
    f = g.Cfr(mode, guard, A, 0, 2)
    assert f.run(x).tobytes() == x.tobytes()
    assert f.read().as_tuple() == (8, 0, 0, 0, 0.0)
    f.close()
    # a threshold above the model's peak
    _, ctr = cr.run(md, x, A, 1, 4)
    high = float(np.float32(1.05 * np.sqrt(ctr["peak_power_in"])))
    f = g.Cfr(mode, guard, high, 4, 4)
    assert f.run(x).tobytes() == x.tobytes()
    r = f.read()
    assert r.as_tuple()[:4] == (8, 0, 0, 0) and abs(r.peak_power_in - ctr["peak_power_in"]) <= 1e-5 * ctr["peak_power_in"]
    f.close()
    # one NaN, in a prefix; an infinity, in a useful part: those symbols come through as they are, their neighbours as the model has them
    y = x.copy()
    y[2 * md.symbol + 3] = np.complex64(complex(np.nan, 0.5))
    y[5 * md.symbol + md.G + 700] = np.complex64(complex(0.1, -np.inf))
    ref, ctr = cr.run(md, y, A, 4, 2)
    f = g.Cfr(mode, guard, A, 4, 2)
    d = Dev(g, y)
    o = Dev(g, n=len(y))
    f.run_device(d.ptr, len(y), o.ptr)
    got, reading = o.get(), f.read()
    for l in range(8):
        sl = slice(l * md.symbol, (l + 1) * md.symbol)
        if l in (2, 5):
            assert got[sl].tobytes() == y[sl].tobytes()
        else:
            assert np.abs(got[sl] - ref[sl]).max() <= 17e-5 * np.abs(ref[sl]).max()
    assert ctr["margin"] > MARGIN and reading.as_tuple()[:4] == _reading(ctr) == (8, 6, 2, ctr["samples_over"])
    # ... and in place
    f.reset()
    f.run_device(d.ptr, len(y), d.ptr)
    assert d.get().tobytes() == got.tobytes() and f.read() == reading
    f.close(); d.free(); o.free()


# ------------------------------------------------------------------ 3. calls, buffers, streams
@pytest.fixture(scope="module")
def whole(g, streams):
    """per shape: (threshold, one host call's output at os 2, 4 iterations, its reading)"""
    out = {}
    for shape in SHAPES:
        mode, guard, md, x, power = streams[shape]
        A = _threshold(md, x, power, 2)
        f = g.Cfr(mode, guard, A)
        out[shape] = (A, f.run(x), f.read())
        f.close()
    return out


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_split_calls_on_two_streams_equal_one_call(g, streams, whole):
    mode, guard, md, x, power = streams["2k"]
    A, ref, reading = whole["2k"]
    dev = torch.device("cuda:0")
    din = torch.from_numpy(x.view(np.float32).copy()).to(dev)
    dout = torch.zeros_like(din)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    f = g.Cfr(mode, guard, A)
    torch.cuda.synchronize()
    p = 0
    for i, nsym in enumerate((1, 3, 4)):
        n = nsym * md.symbol
        f.run_device(din.data_ptr() + 8 * p, n, dout.data_ptr() + 8 * p, stream=(s1, s2)[i & 1].cuda_stream)
        f.run_device(din.data_ptr(), 0, dout.data_ptr(), stream=s1.cuda_stream)          # nothing
        p += n
    assert f.read() == reading                                      # read synchronises with whatever stream ran last
    torch.cuda.synchronize()
    assert dout.cpu().numpy().view(np.complex64).tobytes() == ref.tobytes()
    # the host entry, cut the other way; then a handle that begins at symbol 5
    f.reset()
    assert f.read().as_tuple() == (0, 0, 0, 0, 0.0)
    parts = [f.run(x[:4 * md.symbol]), f.run(x[:0]), f.run(x[4 * md.symbol:7 * md.symbol]), f.run(x[7 * md.symbol:])]
    assert np.concatenate(parts).tobytes() == ref.tobytes() and f.read() == reading
    f.close()
    f = g.Cfr(mode, guard, A, first_symbol=5)
    assert f.run(x[5 * md.symbol:]).tobytes() == ref[5 * md.symbol:].tobytes()
    f.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_in_place_equals_out_of_place_and_guard_floats_stay(g, streams, whole, shape):
    mode, guard, md, x, power = streams[shape]
    A, ref, reading = whole[shape]
    n, pad = len(x), 64
    guard_val = np.full(pad, np.complex64(complex(-7.25, 3.5)))
    buf = Dev(g, n=n + 2 * pad)
    out = Dev(g, n=n + 2 * pad)
    f = g.Cfr(mode, guard, A)
    for d in (buf, out):
        d.put(guard_val, 0); d.put(guard_val, pad + n)
    buf.put(x, pad)
    f.run_device(buf.ptr + 8 * pad, n, out.ptr + 8 * pad)
    o = out.get()
    assert o[pad:pad + n].tobytes() == ref.tobytes()
    assert o[:pad].tobytes() == guard_val.tobytes() and o[pad + n:].tobytes() == guard_val.tobytes()
    assert buf.get(pad, n).tobytes() == x.tobytes(), "the input is read only"
    f.reset()
    f.run_device(buf.ptr + 8 * pad, n, buf.ptr + 8 * pad)           # in place
    b = buf.get()
    assert b[pad:pad + n].tobytes() == ref.tobytes()
    assert b[:pad].tobytes() == guard_val.tobytes() and b[pad + n:].tobytes() == guard_val.tobytes()
    assert f.read() == reading
    f.close(); buf.free(); out.free()


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_two_handles_at_once(g, streams, whole):
    dev = torch.device("cuda:0")
    s = {k: torch.cuda.Stream() for k in SHAPES}
    h, din, dout = {}, {}, {}
    for k in SHAPES:
        mode, guard, md, x, power = streams[k]
        h[k] = g.Cfr(mode, guard, whole[k][0])
        din[k] = torch.from_numpy(x.view(np.float32).copy()).to(dev)
        dout[k] = torch.zeros_like(din[k])
    torch.cuda.synchronize()
    for half in (0, 1):                                             # the two handles' calls interleaved, each on its own stream
        for k in SHAPES:
            n = len(streams[k][3]) // 2
            h[k].run_device(din[k].data_ptr() + 8 * half * n, n, dout[k].data_ptr() + 8 * half * n, stream=s[k].cuda_stream)
    torch.cuda.synchronize()
    for k in SHAPES:
        assert dout[k].cpu().numpy().view(np.complex64).tobytes() == whole[k][1].tobytes(), k
        assert h[k].read() == whole[k][2]
        h[k].close()


def test_refused_calls_leave_the_stream_intact(g, streams, whole):
    mode, guard, md, x, power = streams["2k"]
    A, ref, reading = whole["2k"]
    f = g.Cfr(mode, guard, A)
    L = g.lib()
    din, dout = Dev(g, x), Dev(g, n=len(x))
    S = md.symbol
    f.run_device(din.ptr, 3 * S, dout.ptr)
    before, r0 = dout.get(), f.read()
    run_device = L.dvbt_cfr_run_device
    for inp, n, out in ((din.ptr + 8 * 3 * S, S - 1, dout.ptr + 8 * 3 * S),           # a length that cuts a symbol
                        (din.ptr + 8 * 3 * S, S + 1, dout.ptr + 8 * 3 * S),
                        (din.ptr + 8 * 3 * S, 1, dout.ptr + 8 * 3 * S),
                        (din.ptr + 8 * 3 * S, 2 * S, din.ptr + 8 * 4 * S),            # the output begins inside the input
                        (din.ptr + 8 * 3 * S, 2 * S, din.ptr + 8 * (3 * S - 1)),      # one sample off being in place
                        (din.ptr + 8 * 3 * S + 4, S, dout.ptr + 8 * 3 * S),           # a misaligned buffer
                        (None, S, dout.ptr + 8 * 3 * S),
                        (din.ptr + 8 * 3 * S, S, None)):
        assert run_device(f.h, C.c_void_p(inp), n, C.c_void_p(out), None) == -1
    with pytest.raises(g.DvbtError):
        f.run(x[:S - 1])
    assert din.get().tobytes() == x.tobytes() and dout.get().tobytes() == before.tobytes() and f.read() == r0
    f.run_device(din.ptr + 8 * 3 * S, len(x) - 3 * S, dout.ptr + 8 * 3 * S)             # continues where the last good call ended: symbol 3
    assert dout.get().tobytes() == ref.tobytes() and f.read() == reading
    f.close(); din.free(); dout.free()


# ------------------------------------------------------------------ 4. device-resident loopback
def test_loopback_through_the_receiver_and_the_papr_behind_the_block(g, po):
    """Tx (2k QAM64 7/8, two superframes: the receiver delivers from the second on) -> Cfr at 7 dB, 2x, 4 iterations -> Rx: the transport stream comes
    back as sent.  Spectrum's PAPR at 1e-3 behind the block is lower than in front of it by what the model takes off the same samples, less 0.2 dB."""
    const, cr_, mode = g.QAM64, g.C7_8, g.T2k
    c = po.cfg(const, cr_, mode)
    md = cr.Mode(0, 0)
    ibits = c.payload * c.m * c.k // c.n
    npk = 2 * po.packets_per_superframe(c)
    ts = po.make_ts(npk, 11)
    lead, tail = 1000, 3 * c.N
    L = g.lib()
    tx = g.Tx(const, cr_, mode, scale=po.tx_scale(c), max_packets=npk)
    nbody = tx.samples_for(npk)
    assert nbody % md.symbol == 0
    total = lead + nbody + tail
    dts = L.dvbt_device_malloc(len(ts) + 64)
    assert L.dvbt_copy_to_device(C.c_void_p(dts), ts.ctypes.data_as(C.c_void_p), len(ts)) == 0
    a, b = Dev(g, n=total), Dev(g, n=total)
    assert tx.run_device(dts, npk, a.ptr + 8 * lead, nbody) == nbody
    meter = g.Channel()
    power = meter.power(a.ptr + 8 * lead, nbody)
    A = g.Cfr.threshold_for(PAPR_DB, power)
    f = g.Cfr(mode, g.G1_32, A, 4, 2)
    f.run_device(a.ptr + 8 * lead, nbody, b.ptr + 8 * lead)          # (lead-in and tail of b stay zero, as a's are)
    reading = f.read()
    assert reading.symbols == nbody // md.symbol and reading.symbols_nonfinite == 0 and reading.symbols_clipped > 0.9 * reading.symbols
    papr = []
    spec = g.Spectrum(1024, 512, "hann")
    for d in (a, b):
        spec.reset()
        spec.push_device(d.ptr + 8 * lead, nbody)
        papr.append(spec.read().papr_db(1e-3))
    x = a.get(lead, nbody)
    ref, _ = cr.run(md, x, float(np.float32(A)), 4, 2)
    model_cut = cr.papr_db(x, 1e-3) - cr.papr_db(ref, 1e-3)
    print(f"\nPAPR at 1e-3: {papr[0]:.2f} dB in front, {papr[1]:.2f} dB behind; the model takes {model_cut:.2f} dB off; highest first-iteration peak "
          f"{reading.peak_db(power):.2f} dB; {reading}")
    assert model_cut > 1.0
    assert papr[0] - papr[1] >= model_cut - 0.2
    rx = g.Rx(const, cr_, mode, max_samples=total, taps=True)
    rep = rx.run_device(b.ptr, total)
    assert rep.n_lock_periods == 1
    got_ts = rx.tap(g.TAP_TS)
    p0 = rep.first_out_symbol * ibits // 8 // 204 + rep.ts_first_packet - 11
    n = len(got_ts) // 188
    assert n > 0 and p0 >= 0 and p0 + n <= npk
    assert (got_ts.reshape(-1, 188) == ts.reshape(-1, 188)[p0:p0 + n]).all()
    rx.close(); tx.close(); f.close(); meter.close(); spec.close()
    a.free(); b.free(); L.dvbt_device_free(C.c_void_p(dts))
