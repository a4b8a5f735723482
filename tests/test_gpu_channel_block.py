"""The GPU channel block (dvbt_channel_*, gr_dvbt_amd.Channel) against its numpy model tests/chanref.py and the oracle's test channel po.channel.

TOL: 1e-5 of the model's peak sample, the project's bound for a float32 baseband (test_gpu_tx._close); the kernel's own error is a few 1e-7 (the float
rounding of a sample's two or three operations, 2e-8 rad of phase).  What a stream looks like cut into calls, run through the host or the device entry,
or run again after a reset is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import chanref

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

SEEDS = (5, 0x0123456789abcdef)
FAR = 2 ** 40 + 3
ECHOES = ((57, 0.15), (19, -0.1j))
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


def _within_tol(got, model):
    assert got.shape == model.shape and got.dtype == np.complex64 and len(model) > 0
    err, peak = np.abs(got - model).max(), np.abs(model).max()
    print(f"\nlargest error {err:.3e} = {err / peak:.2e} of the peak {peak:.4f}")
    assert err <= 1e-5 * peak


@pytest.fixture(scope="module")
def stream2k(po):
    """(configuration, one superframe of 2k QAM16 1/2 behind 1000 zeros)"""
    c = po.cfg(po.QAM16, po.C1_2, po.T2k)
    return c, po.tx(c, po.make_ts(po.packets_per_superframe(c), 3), lead_in=1000, tail=3 * c.N)


@pytest.fixture(scope="module")
def random_x():
    rng = np.random.RandomState(17)
    x = (rng.randn((1 << 20) + 1) + 1j * rng.randn((1 << 20) + 1)).astype(np.complex64)
    x[0] = complex(-0.0, 0.0)
    return x


# ------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 4097, (1 << 20) + 1])
def test_identity_is_bit_exact(g, random_x, n):
    ch = g.Channel()
    x = random_x[:n]
    assert ch.run(x).tobytes() == x.tobytes()
    assert ch.run(x).tobytes() == x.tobytes()                      # and again, from wherever the first call left the stream (an odd index for odd n)
    ch.close()


# ------------------------------------------------------------------ 2. noise alone
@pytest.fixture(scope="module")
def model_noise():
    cache = {}

    def get(seed, first, n):
        if (seed, first, n) not in cache:
            cache[(seed, first, n)] = chanref.noise(seed, first, n)
        return cache[(seed, first, n)]
    return get


@pytest.mark.parametrize("first,n", [(0, (1 << 20) + 1), (FAR, 4097)])
@pytest.mark.parametrize("seed", SEEDS)
def test_noise_alone(g, model_noise, seed, first, n):
    zeros = np.zeros(n, np.complex64)
    a = g.Channel(noise_sigma=1.0, seed=seed, first_sample=first)
    b = g.Channel(noise_sigma=1.0, seed=seed, first_sample=first)
    ya, yb = a.run(zeros), b.run(zeros)
    _within_tol(ya, model_noise(seed, first, n))
    assert ya.tobytes() == yb.tobytes()
    other = g.Channel(noise_sigma=1.0, seed=seed + 1, first_sample=first)
    yo = other.run(zeros)
    assert (yo != ya).mean() > 0.999
    _within_tol(yo, model_noise(seed + 1, first, n))
    a.close(); b.close(); other.close()


# ------------------------------------------------------------------ 3. echoes and offset
def test_echoes_and_offset_against_the_oracles_channel(g, po, stream2k):
    c, iq = stream2k
    ch = g.Channel(echoes=ECHOES, cfo=3.37, fft_length=c.N)
    got = ch.run(iq)
    ch.close()
    _within_tol(got, po.channel(iq, c.N, cfo=3.37, echoes=ECHOES).astype(np.complex128))
    _within_tol(got, chanref.channel(iq, echoes=ECHOES, cfo=3.37, fft_length=c.N))


def test_longest_and_shortest_delay_far_into_a_stream(g, stream2k):
    c, iq = stream2k
    x = iq[900:60900]
    echoes = ((8192, 0.2 + 0.1j), (1, -0.1j))
    ch = g.Channel(echoes=echoes, cfo=-7.63, fft_length=c.N, first_sample=FAR)
    got = ch.run(x)
    ch.close()
    _within_tol(got, chanref.channel(x, echoes=echoes, cfo=-7.63, fft_length=c.N, first_sample=FAR))


# ------------------------------------------------------------------ 4. splits
ALL_ON = dict(echoes=((1, -0.1j), (57, 0.15), (8192, 0.2 + 0.1j)), cfo=3.37, fft_length=2048, noise_sigma=0.01)
SPLITS = [1, 7, 0, 1000, 8191, 8192, 8193]
N_SPLIT = 50001


def _cuts(n):
    sizes = SPLITS + [n - sum(SPLITS)]
    assert sizes[-1] > 0
    return sizes


@pytest.mark.parametrize("first", [0, FAR])
def test_split_calls_equal_one_call_bit_for_bit(g, stream2k, first):
    x = stream2k[1][900:900 + N_SPLIT]
    ch = g.Channel(seed=5, first_sample=first, **ALL_ON)
    whole = ch.run(x)
    _within_tol(whole, chanref.channel(x, seed=5, first_sample=first, **ALL_ON))
    # the host entry, cut
    ch.reset()
    parts, p = [], 0
    for n in _cuts(len(x)):
        parts.append(ch.run(x[p:p + n]))
        assert len(parts[-1]) == n
        p += n
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    # the device entry, cut the same way, on the default stream
    ch.reset()
    din, dout = Dev(g, x), Dev(g, n=len(x))
    p = 0
    for n in _cuts(len(x)):
        ch.run_device(din.ptr + 8 * p, n, dout.ptr + 8 * p)
        p += n
    assert dout.get().tobytes() == whole.tobytes()
    # after a reset: the same bytes again, in one device call
    ch.reset()
    dout.put(np.zeros(len(x), np.complex64))
    ch.run_device(din.ptr, len(x), dout.ptr)
    assert dout.get().tobytes() == whole.tobytes()
    # a fresh handle that starts where a cut would: the second half alone, with the first half's tail as its history's only gap
    half = 20001
    tail = g.Channel(seed=5, first_sample=first + half, **ALL_ON).run(x[half:])
    assert tail[8192:].tobytes() == whole[half + 8192:].tobytes()
    din.free(); dout.free(); ch.close()


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_device_entry_on_two_streams(g, stream2k):
    x1 = stream2k[1][900:900 + N_SPLIT]
    x2 = stream2k[1][30000:30000 + N_SPLIT]
    ra, rb = g.Channel(seed=5, **ALL_ON), g.Channel(seed=6, first_sample=FAR, **ALL_ON)
    ref1, ref2 = ra.run(x1), rb.run(x2)
    ra.close(); rb.close()
    dev = torch.device("cuda:0")
    d1, d2 = torch.from_numpy(x1.view(np.float32).copy()).to(dev), torch.from_numpy(x2.view(np.float32).copy()).to(dev)
    o1, o2 = torch.zeros_like(d1), torch.zeros_like(d2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = g.Channel(seed=5, **ALL_ON), g.Channel(seed=6, first_sample=FAR, **ALL_ON)
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


# ------------------------------------------------------------------ 5. power
@pytest.mark.parametrize("n", [1, 65, (1 << 20) + 1])
def test_power(g, random_x, n):
    x = random_x[-n:] * np.float32(0.37)                    # (not the zero at the front: a lone zero sample has no relative error)
    assert len(x) == n
    want = np.mean(np.abs(x.astype(np.complex128)) ** 2)
    ch = g.Channel()
    d = Dev(g, x)
    p1, p2 = ch.power(d.ptr, n), ch.power(d.ptr, n)
    print(f"\npower {p1!r}, numpy {want!r}: {abs(p1 - want) / want:.2e} relative")
    assert abs(p1 - want) <= 1e-6 * want
    assert np.float64(p1).tobytes() == np.float64(p2).tobytes()
    with pytest.raises(g.DvbtError):
        ch.power(d.ptr, 0)
    d.free(); ch.close()


# ------------------------------------------------------------------ 6. errors
def test_refused_calls_leave_the_stream_intact(g, stream2k):
    x = stream2k[1][900:900 + 20000]
    ch = g.Channel(seed=5, **ALL_ON)
    whole = ch.run(x)
    ch.reset()
    L = g.lib()
    din, dout = Dev(g, x), Dev(g, n=len(x))
    ch.run_device(din.ptr, 1001, dout.ptr)
    before = dout.get()
    run_device = L.dvbt_channel_run_device
    for inp, n, out in ((din.ptr + 8 * 1001, 100, din.ptr + 8 * 1011),            # the output begins inside the input
                        (din.ptr + 8 * 1001, 100, din.ptr + 8 * 1001),            # in place
                        (din.ptr + 8 * 1001, 100, din.ptr + 8 * 902),             # the output ends inside the input
                        (din.ptr + 8 * 1001 + 4, 100, dout.ptr + 8 * 1001),       # a misaligned buffer
                        (din.ptr, 2 ** 31 + 1, dout.ptr),                         # more than a call takes (refused before anything is read)
                        (None, 100, dout.ptr + 8 * 1001)):
        assert run_device(ch.h, C.c_void_p(inp), n, C.c_void_p(out), None) == -1
    with pytest.raises(g.DvbtError):
        ch.run_device(din.ptr + 8 * 1001, 100, din.ptr + 8 * 1011)
    assert din.get().tobytes() == x.tobytes() and dout.get().tobytes() == before.tobytes()
    ch.run_device(din.ptr + 8 * 1001, len(x) - 1001, dout.ptr + 8 * 1001)          # continues where the last good call ended
    assert dout.get().tobytes() == whole.tobytes()
    din.free(); dout.free(); ch.close()


# ------------------------------------------------------------------ 7. device-resident loopback
@pytest.mark.parametrize("seed", SEEDS)
def test_loopback_that_never_leaves_the_device(g, po, seed):
    const, cr, mode, nsf, snr = g.QAM16, g.C1_2, g.T2k, 2, 20.0
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
    clean = g.Channel(echoes=ECHOES, cfo=3.37, fft_length=c.N)
    clean.run_device(a.ptr, total, b.ptr)
    sigma = g.Channel.sigma(snr, clean.power(b.ptr + 8 * 1000, 100000))
    noisy = g.Channel(echoes=ECHOES, cfo=3.37, fft_length=c.N, noise_sigma=sigma, seed=seed)
    noisy.run_device(a.ptr, total, y.ptr)
    rx = g.Rx(const, cr, mode, max_samples=total, snr_db=snr, taps=True)
    rep = rx.run_device(y.ptr, total)
    assert rep.n_lock_periods == 1
    got_ts = rx.tap(g.TAP_TS)
    p0 = rep.first_out_symbol * ibits // 8 // 204 + rep.ts_first_packet - 11
    n = len(got_ts) // 188
    assert n > 0 and p0 >= 0 and p0 + n <= npk
    assert (got_ts.reshape(-1, 188) == ts.reshape(-1, 188)[p0:p0 + n]).all()
    # the same samples on the host: what the model says they are, and what the oracle's receiver makes of them
    host = y.get()
    ref_power = np.mean(np.abs(b.get(1000, 100000).astype(np.complex128)) ** 2)
    assert abs(sigma - np.sqrt(ref_power / 10 ** (snr / 10) / 2)) <= 1e-6 * sigma
    _within_tol(host, chanref.channel(a.get(), echoes=ECHOES, cfo=3.37, fft_length=c.N, noise_sigma=sigma, seed=seed))
    o = po.rx(c, host, snr_db=snr, want=INT_TAPS)
    assert o["truncated"] == 0 and rep.first_out_symbol == o["first_out_symbol"]
    for name in INT_TAPS:
        x, r = rx.tap(getattr(g, "TAP_" + {"vit": "VITERBI"}.get(name, name.upper()))), o[name]
        assert x.size == r.size > 0, name
        assert (x.reshape(-1) == r.reshape(-1)).all(), name
    assert rep.rs_fail_words == o["rs_fail"] and rep.rs_corrected_symbols == o["rs_corr"]
    rx.close(); tx.close(); clean.close(); noisy.close()
    a.free(); b.free(); y.free(); L.dvbt_device_free(C.c_void_p(dts))


# ------------------------------------------------------------------ 8. noise level through the receiver
@pytest.mark.parametrize("const,cr,nsf,snr", [(1, 0, 4, 12.0), (2, 4, 2, 24.0)], ids=["2k_qam16_1_2_12dB", "2k_qam64_7_8_24dB"])
def test_noise_level_through_the_receiver(g, po, const, cr, nsf, snr):
    """MER of the same receiver on the block's noise and on po.channel's (numpy's generator, seed 5) at the same sigma: two realisations over >= 4e5 cells
    differ by about 0.01 dB, a sigma wrong by sqrt(2) by 3 dB"""
    c = po.cfg(const, cr, po.T2k)
    iq = po.stream_slice(c, nsf, 9)
    ref = po.channel(iq, c.N, snr_db=snr, seed=5)
    d = Dev(g, iq)
    sigma = g.Channel.sigma(snr, g.Channel().power(d.ptr + 8 * 1000, 100000))
    d.free()
    want_sigma = np.sqrt(np.mean(np.abs(iq[1000:101000].astype(np.complex128)) ** 2) / 10 ** (snr / 10) / 2)
    assert abs(sigma - want_sigma) <= 1e-6 * want_sigma
    got = g.Channel(noise_sigma=sigma, seed=5).run(iq)
    mer = []
    for y in (got, ref):
        rx = g.Rx(const, cr, g.T2k, max_samples=len(iq), snr_db=snr, quality=True)
        rx.run(y)
        q = rx.quality()
        assert q.mer_carriers >= 4e5
        mer.append(q.mer_db)
        rx.close()
    print(f"\nMER on the block's noise {mer[0]:.4f} dB, on numpy's {mer[1]:.4f} dB")
    assert abs(mer[0] - mer[1]) < 0.1
