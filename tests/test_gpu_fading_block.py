"""The GPU fading block (dvbt_fading_*, gr_dvbt_amd.Fading) against its numpy model tests/fadingref.py.

TOL: 1e-5 of the model's peak sample, the project's bound for a float32 baseband (test_gpu_channel_block._within_tol); the kernel's own error is the float
rounding of a knot's M additions and a sample's few operations.  What a stream looks like cut into calls, run through the host or the device entry, run
again after a reset or begun later by a second handle is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import chanref
import fadingref as fr

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

SEEDS = (5, 0x0123456789abcdef)
FAR = 2 ** 40 + 3
INT_TAPS = ("demap", "symdeint", "bitdeint", "vit", "deint", "rs", "ts")


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
        assert self.ptr
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


def _within_tol(got, model, extra=0.0):
    assert got.shape == model.shape and got.dtype == np.complex64 and len(model) > 0
    err, peak = np.abs(got - model).max(), np.abs(model).max()
    print(f"\nlargest error {err:.3e} = {err / peak:.2e} of the peak {peak:.4f} (allowed beyond 1e-5 of it: {extra:.3e})")
    assert err <= 1e-5 * peak + extra


@pytest.fixture(scope="module")
def stream2k(po):
    """(configuration, one superframe of 2k QAM16 1/2 behind 1000 zeros): test_gpu_channel_block's"""
    c = po.cfg(po.QAM16, po.C1_2, po.T2k)
    return c, po.tx(c, po.make_ts(po.packets_per_superframe(c), 3), lead_in=1000, tail=3 * c.N)


@pytest.fixture(scope="module")
def random_x():
    rng = np.random.RandomState(23)
    return (rng.randn((1 << 16) + 1) + 1j * rng.randn((1 << 16) + 1)).astype(np.complex64)


# ------------------------------------------------------------------ 1. one static path
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 4097, (1 << 16) + 1])
def test_one_static_path_gives_the_input(g, random_x, n):
    f = g.Fading(paths=((0, 1.0, 0.0),))
    x = random_x[:n]
    a = f.run(x)
    b = f.run(x)                                   # and again, from wherever the first call left the stream (an odd index for odd n)
    assert a.dtype == np.complex64 and a.shape == x.shape
    assert np.array_equal(a, x) and np.array_equal(b, x)
    f.close()


# ------------------------------------------------------------------ 2. the gains, read back
@pytest.mark.parametrize("first", [0, FAR])
@pytest.mark.parametrize("doppler", [2.0 ** -16, 2.0 ** -12])
@pytest.mark.parametrize("M", [1, 16, 32])
def test_gains_read_back(g, M, doppler, first):
    n = 4097
    paths = ((0, 0.0, 1.0),)
    ones = np.ones(n, np.complex64)
    f = g.Fading(paths=paths, doppler=doppler, n_sinusoids=M, seed=5, first_sample=first)
    got = f.run(ones)
    f.close()
    p = fr.params(paths, doppler, M, 5)
    _within_tol(got, fr.gains(p, first, n)[0])
    _within_tol(got, fr.exact_gains(p, first, n)[0], extra=fr.chord_bound(p, 0))
    o = g.Fading(paths=paths, doppler=doppler, n_sinusoids=M, seed=6, first_sample=first)
    other = o.run(ones)
    o.close()
    assert (other != got).mean() > 0.999
    _within_tol(other, fr.gains(fr.params(paths, doppler, M, 6), first, n)[0])


# ------------------------------------------------------------------ 3. everything at once
def _paths24():
    delays = [0, 1, 8192, 57, 57, 2, 3, 63, 64, 65, 127, 500, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 19, 46, 5, 15]
    rng = np.random.RandomState(3)
    out = []
    for i, d in enumerate(delays):
        los = complex(0.3 * rng.randn(), 0.3 * rng.randn()) if i % 3 != 1 else 0.0      # fixed and scattered parts mixed: both, scatter only, fixed only
        sg = 0.0 if i % 3 == 2 else 0.1 + 0.05 * i
        out.append((d, los, sg))
    return tuple(out)


PATHS24 = _paths24()


@pytest.mark.parametrize("first", [0, FAR])
def test_everything_at_once(g, random_x, first):
    assert len(PATHS24) == 24
    x = random_x[:20000]
    f = g.Fading(paths=PATHS24, doppler=1e-4, n_sinusoids=32, seed=SEEDS[1], first_sample=first)
    got = f.run(x)
    f.close()
    _within_tol(got, fr.fading(x, fr.params(PATHS24, 1e-4, 32, SEEDS[1]), first))


# ------------------------------------------------------------------ 4. TU6
def test_tu6_on_a_superframe(g, stream2k):
    c, iq = stream2k
    f = g.Fading.tu6(100.0, seed=5)
    got = f.run(iq)
    f.close()
    paths, dop = fr.tu6(100.0)
    assert dop == f.p.doppler and [f.p.delay[i] for i in range(6)] == [0, 2, 5, 15, 21, 46] and f.p.n_paths == 6
    _within_tol(got, fr.fading(iq, fr.params(paths, dop, 16, 5)))


# ------------------------------------------------------------------ 5. splits
MIXED = dict(paths=((0, 0.8, 0.3), (1, 0.0, 0.5), (57, 0.15j, 0.0), (57, 0.0, 0.2), (8192, 0.2 + 0.1j, 0.4)), doppler=1e-4, n_sinusoids=16)
SPLITS = [1, 2, 61, 64, 67, 255, 257, 1000, 8191, 8193]
N_SPLIT = 40001


def _cuts(n):
    sizes = SPLITS + [n - sum(SPLITS)]
    assert sizes[-1] > 0
    return sizes


@pytest.fixture(scope="module")
def whole_runs(g, random_x):
    """first -> the one-call output of the MIXED block on random_x[:N_SPLIT], checked against the model once"""
    out = {}
    for first in (0, FAR):
        f = g.Fading(seed=5, first_sample=first, **MIXED)
        out[first] = f.run(random_x[:N_SPLIT])
        f.close()
        _within_tol(out[first], fr.fading(random_x[:N_SPLIT], fr.params(MIXED["paths"], MIXED["doppler"], 16, 5), first))
    return out


@pytest.mark.parametrize("first", [0, FAR])
def test_split_calls_equal_one_call_bit_for_bit(g, random_x, whole_runs, first):
    x, whole = random_x[:N_SPLIT], whole_runs[first]
    f = g.Fading(seed=5, first_sample=first, **MIXED)
    # the host entry, cut
    parts, p = [], 0
    for n in _cuts(len(x)):
        parts.append(f.run(x[p:p + n]))
        assert len(parts[-1]) == n
        p += n
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    # the device entry, cut the same way, on the default stream
    f.reset()
    din, dout = Dev(g, x), Dev(g, n=len(x))
    p = 0
    for n in _cuts(len(x)):
        f.run_device(din.ptr + 8 * p, n, dout.ptr + 8 * p)
        p += n
    assert dout.get().tobytes() == whole.tobytes()
    # after a reset: the same bytes again, in one device call
    f.reset()
    dout.put(np.zeros(len(x), np.complex64))
    f.run_device(din.ptr, len(x), dout.ptr)
    assert dout.get().tobytes() == whole.tobytes()
    din.free(); dout.free(); f.close()


# ------------------------------------------------------------------ 6. a handle that begins later
@pytest.mark.parametrize("first", [0, FAR])
def test_a_later_handle_continues_the_stream(g, random_x, whole_runs, first):
    s = 20001
    assert s % 2 == 1 and (first + s) % 64 != 0
    f = g.Fading(seed=5, first_sample=first + s, **MIXED)
    tail = f.run(random_x[s:N_SPLIT])
    f.close()
    assert tail[8192:].tobytes() == whole_runs[first][s + 8192:].tobytes()


# ------------------------------------------------------------------ 7. two streams
@pytest.mark.skipif(torch is None, reason="needs torch")
def test_device_entry_on_two_streams(g, random_x, whole_runs):
    x1, x2 = random_x[:N_SPLIT], random_x[20000:20000 + N_SPLIT]
    r = g.Fading(seed=6, first_sample=FAR, **MIXED)
    ref1, ref2 = whole_runs[0], r.run(x2)
    r.close()
    dev = torch.device("cuda:0")
    d1, d2 = torch.from_numpy(x1.view(np.float32).copy()).to(dev), torch.from_numpy(x2.view(np.float32).copy()).to(dev)
    o1, o2 = torch.zeros_like(d1), torch.zeros_like(d2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = g.Fading(seed=5, **MIXED), g.Fading(seed=6, first_sample=FAR, **MIXED)
    torch.cuda.synchronize()
    # two handles interleaved on two streams, each in three calls; handle a changes streams between its calls
    cuts = [0, 9001, 9002, N_SPLIT]
    for i in range(3):
        lo, hi = cuts[i], cuts[i + 1]
        sa = s1 if i != 1 else s2
        a.run_device(d1.data_ptr() + 8 * lo, hi - lo, o1.data_ptr() + 8 * lo, stream=sa.cuda_stream)
        b.run_device(d2.data_ptr() + 8 * lo, hi - lo, o2.data_ptr() + 8 * lo, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert o1.cpu().numpy().view(np.complex64).tobytes() == ref1.tobytes()
    assert o2.cpu().numpy().view(np.complex64).tobytes() == ref2.tobytes()
    a.close(); b.close()


# ------------------------------------------------------------------ 8. errors
def test_refused_calls_leave_the_stream_intact(g, random_x, whole_runs):
    x = random_x[:20000]
    whole = whole_runs[0][:20000]                                                  # a causal block: the first 20000 outputs of the longer run
    f = g.Fading(seed=5, **MIXED)
    L = g.lib()
    din, dout = Dev(g, x), Dev(g, n=len(x))
    f.run_device(din.ptr, 1001, dout.ptr)
    before = dout.get()
    run_device = L.dvbt_fading_run_device
    for inp, n, out in ((din.ptr + 8 * 1001, 100, din.ptr + 8 * 1011),            # the output begins inside the input
                        (din.ptr + 8 * 1001, 100, din.ptr + 8 * 1001),            # in place
                        (din.ptr + 8 * 1001, 100, din.ptr + 8 * 902),             # the output ends inside the input
                        (din.ptr + 8 * 1001 + 4, 100, dout.ptr + 8 * 1001),       # a misaligned buffer
                        (din.ptr, 2 ** 31 + 1, dout.ptr),                         # more than a call takes (refused before anything is read)
                        (None, 100, dout.ptr + 8 * 1001)):
        assert run_device(f.h, C.c_void_p(inp), n, C.c_void_p(out), None) == -1
    with pytest.raises(g.DvbtError):
        f.run_device(din.ptr + 8 * 1001, 100, din.ptr + 8 * 1011)
    assert din.get().tobytes() == x.tobytes() and dout.get().tobytes() == before.tobytes()
    f.run_device(din.ptr + 8 * 1001, len(x) - 1001, dout.ptr + 8 * 1001)           # continues where the last good call ended
    assert dout.get().tobytes() == whole.tobytes()
    din.free(); dout.free(); f.close()


# ------------------------------------------------------------------ 9. device-resident loopback
@pytest.mark.parametrize("const,cr,snr,seed", [(1, 0, 20.0, SEEDS[0]), (2, 4, 30.0, SEEDS[1])], ids=["2k_qam16_1_2_20dB", "2k_qam64_7_8_30dB"])
def test_loopback_that_never_leaves_the_device(g, po, const, cr, snr, seed):
    """Tx -> Fading.tu6(100 Hz, Rice K = 10 dB) -> Channel(noise) -> Rx.  The model chain with these seeds gives the oracle one lock period and every
    delivered packet right on the CPU (QAM16: 0 corrected RS symbols; QAM64 7/8: 14)."""
    mode, nsf = g.T2k, 2
    c = po.cfg(const, cr, mode)
    ibits = c.payload * c.m * c.k // c.n
    npk = nsf * po.packets_per_superframe(c)
    ts = po.make_ts(npk, 11)
    lead, tail = 1000, 3 * c.N
    L = g.lib()
    tx = g.Tx(const, cr, mode, scale=po.tx_scale(c), max_packets=npk)
    nbody = tx.samples_for(npk)
    total = lead + nbody + tail
    dts = L.dvbt_device_malloc(len(ts) + 64)
    assert L.dvbt_copy_to_device(C.c_void_p(dts), ts.ctypes.data_as(C.c_void_p), len(ts)) == 0
    a, b, y = Dev(g, n=total), Dev(g, n=total), Dev(g, n=total)
    assert tx.run_device(dts, npk, a.ptr + 8 * lead, nbody) == nbody
    fade = g.Fading.tu6(100.0, rice_k_db=10.0, seed=seed)
    fade.run_device(a.ptr, total, b.ptr)
    meter = g.Channel()
    sigma = g.Channel.sigma(snr, meter.power(b.ptr + 8 * 1000, 100000))
    noisy = g.Channel(noise_sigma=sigma, seed=seed)                               # the same seed: the table's counters are not the noise's
    noisy.run_device(b.ptr, total, y.ptr)
    rx = g.Rx(const, cr, mode, max_samples=total, snr_db=snr, taps=True)
    rep = rx.run_device(y.ptr, total)
    assert rep.n_lock_periods == 1
    got_ts = rx.tap(g.TAP_TS)
    p0 = rep.first_out_symbol * ibits // 8 // 204 + rep.ts_first_packet - 11
    n = len(got_ts) // 188
    assert n > 0 and p0 >= 0 and p0 + n <= npk
    assert (got_ts.reshape(-1, 188) == ts.reshape(-1, 188)[p0:p0 + n]).all()
    # the same samples on the host: what the two models chained say they are, and what the oracle's receiver makes of them
    host, faded = y.get(), b.get()
    paths, dop = fr.tu6(100.0, rice_k_db=10.0)
    model_faded = fr.fading(a.get(), fr.params(paths, dop, 16, seed))
    _within_tol(faded, model_faded)
    ref_power = np.mean(np.abs(faded[1000:101000].astype(np.complex128)) ** 2)
    assert abs(sigma - np.sqrt(ref_power / 10 ** (snr / 10) / 2)) <= 1e-6 * sigma
    _within_tol(host, chanref.channel(model_faded, noise_sigma=sigma, seed=seed))
    o = po.rx(c, host, snr_db=snr, want=INT_TAPS)
    assert o["truncated"] == 0 and rep.first_out_symbol == o["first_out_symbol"]
    for name in INT_TAPS:
        x, r = rx.tap(getattr(g, "TAP_" + {"vit": "VITERBI"}.get(name, name.upper()))), o[name]
        assert x.size == r.size > 0, name
        assert (x.reshape(-1) == r.reshape(-1)).all(), name
    assert rep.rs_fail_words == o["rs_fail"] and rep.rs_corrected_symbols == o["rs_corr"]
    rx.close(); tx.close(); fade.close(); meter.close(); noisy.close()
    a.free(); b.free(); y.free(); L.dvbt_device_free(C.c_void_p(dts))
