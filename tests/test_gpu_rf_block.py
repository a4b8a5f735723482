"""The GPU RF front-end block (dvbt_rf_*, gr_dvbt_amd.RfFrontend) against its numpy model tests/rfref.py.

TOL: 1e-5 of the model's peak sample, the project's bound for a float32 baseband (test_gpu_channel_block._within_tol); the kernel's own error is the float
rounding of a sample's operations, of the 32 additions of the tones' sum and 2e-7 rad of the angle's conversion to turns.  What a stream looks like cut
into calls, shifted by a sample in memory, run in place, through the host or the device entry, run again after a reset or begun later by a second handle is
compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import chanref
import rfref as rr

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

SEEDS = (5, 0x0123456789abcdef)
FAR = 2 ** 40 + 3
INT_TAPS = ("demap", "symdeint", "bitdeint", "vit", "deint", "rs", "ts")
N = (1 << 16) + 1
MASK_20 = ((100.0, -60.0), (1e3, -70.0), (1e4, -80.0), (1e5, -100.0), (1e6, -120.0))     # 1.9 degrees rms
MASK_30 = tuple((f, d - 10.0) for f, d in MASK_20)                                        # 0.6 degrees rms
A_SAT = 1.25


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


def _within_tol(got, model):
    assert got.shape == model.shape and got.dtype == np.complex64 and len(model) > 0
    err, peak = np.abs(got - model).max(), np.abs(model).max()
    print(f"\nlargest error {err:.3e} = {err / peak:.2e} of the peak {peak:.4f}")
    assert err <= 1e-5 * peak


@pytest.fixture(scope="module")
def random_x():
    rng = np.random.RandomState(29)
    return (rng.randn(N) + 1j * rng.randn(N)).astype(np.complex64)


def _all_on(g, seed=5):
    """every stage on, as (the keyword arguments of RfFrontend, the model's Params)"""
    tones = g.phase_noise_tones(MASK_20, 32, seed)
    mu, nu = g.RfFrontend.iq_imbalance(0.5, 3.0)
    kw = dict(sat_amplitude=A_SAT, smoothness=2.0, tones=tones, mu=mu, nu=nu, dc=0.03 - 0.02j)
    return kw, rr.params(**kw)


# ------------------------------------------------------------------ 1. all off
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 65537])
def test_all_off_gives_the_input_bit_for_bit(g, random_x, n):
    f = g.RfFrontend()
    x = random_x[:n].copy()
    if n > 4:
        x[1], x[3] = complex(-0.0, 0.0), complex(np.float32(1e-42), -np.float32(1e-45))      # a negative zero and denormals are bits too
    a = f.run(x)
    b = f.run(x)                                   # and again, from wherever the first call left the stream (an odd index for odd n)
    assert a.dtype == np.complex64 and a.shape == x.shape
    assert a.tobytes() == x.tobytes() and b.tobytes() == x.tobytes()
    z = g.RfFrontend(mu=0, first_sample=FAR)       # a zeroed struct's mu
    assert z.run(x).tobytes() == x.tobytes()
    f.close(); z.close()


def test_all_off_in_place(g, random_x):
    f = g.RfFrontend()
    d = Dev(g, random_x)
    f.run_device(d.ptr, N, d.ptr)
    f.run_device(d.ptr + 8, N - 1, d.ptr + 8)      # and from an address that is not 16-byte aligned
    assert d.get().tobytes() == random_x.tobytes()
    d.free(); f.close()


# ------------------------------------------------------------------ 2. each stage alone
@pytest.fixture(scope="module")
def ramp():
    """amplitudes from 0 to 1000 A at turning angles: (|x| / A)^(2p) overflows a float from 20 A on where p = 16"""
    r = np.linspace(0.0, 1000.0 * A_SAT, N)
    r[1::512] = A_SAT                              # and the knee itself
    return (r * np.exp(0.37j * np.arange(N))).astype(np.complex64)


@pytest.mark.parametrize("first", [0, FAR])
@pytest.mark.parametrize("p", [0.5, 2.0, 16.0])
def test_the_amplifier_alone(g, random_x, ramp, p, first):
    f = g.RfFrontend(sat_amplitude=A_SAT, smoothness=p, first_sample=first)
    got_ramp, got_rand = f.run(ramp), f.run(random_x)
    f.close()
    assert np.isfinite(got_ramp.view(np.float32)).all() and got_ramp[0] == 0
    assert np.abs(got_ramp).max() <= A_SAT * (1 + 2e-7)
    _within_tol(got_ramp, rr.pa(ramp, A_SAT, p))
    _within_tol(got_rand, rr.pa(random_x, A_SAT, p))
    turn = np.angle(got_ramp[1:].astype(np.complex128) * np.conj(ramp[1:].astype(np.complex128)))
    assert np.abs(turn).max() <= 3e-7                                                # the phase is untouched


def test_the_amplifier_at_the_ends_of_the_floats(g):
    x = np.array([0, -0.0, 1e-45, 1e-40 - 1e-41j, 1e-30j, 3e38 + 3e38j, -3.4e38, 1e19 - 1e19j, 2e19j], dtype=np.complex64)
    for A in (1e-30, 1.0, 1e30):
        f = g.RfFrontend(sat_amplitude=A, smoothness=16.0)
        got = f.run(x)
        f.close()
        assert np.isfinite(got.view(np.float32)).all()
        model = rr.pa(x, float(np.float32(A)), 16.0)
        err = np.abs(got - model)
        print(A, "largest error relative to each sample's model:", (err[2:] / np.abs(model[2:])).max())
        assert (err <= 1e-5 * np.abs(model) + 1e-45).all()                              # each sample against its own size: they span 80 decades
        assert got[0] == 0 and got[1] == 0 and np.signbit(got[1].real)


@pytest.mark.parametrize("first", [0, FAR])
@pytest.mark.parametrize("M", [1, 8, 32])
def test_the_tones_alone(g, M, first):
    tones = g.phase_noise_tones(MASK_20, M, 5)
    tones = (tones[0], tones[1], tones[2] * np.float32(3.0 / tones[2].astype(np.float64).sum()))      # louder than any oscillator: sum a = 3 rad
    assert float(tones[2].astype(np.float64).sum()) <= np.pi
    f = g.RfFrontend(tones=tones, first_sample=first)
    got = f.run(np.ones(N, np.complex64))
    f.close()
    p = rr.params(tones=tones)
    phi = rr.phi(p.tones, first, N)
    assert np.abs(phi).max() > 0.5
    _within_tol(got, np.exp(1j * phi))
    # the model's phases once more in Python integers, where the stream is far along
    inc, ph, amp = p.tones
    for j in (0, 1, N - 1):
        want = sum(amp[m] * np.sin(2 * np.pi * ((((ph[m] + inc[m] * (first + j)) % 2 ** 64) >> 32) / 2.0 ** 32)) for m in range(M))
        assert abs(phi[j] - want) <= 1e-12
    o = g.RfFrontend(tones=g.phase_noise_tones(MASK_20, M, 6), first_sample=first)
    other = o.run(np.ones(N, np.complex64))
    o.close()
    assert (other != got).mean() > 0.999


def test_a_spur_list_at_the_largest_angle(g):
    """one tone of amplitude float32(3.1415925) <= pi at a quarter of the sample rate: phi = +-a on the odd samples, the angle's conversion at its ends"""
    a = np.float32(3.1415925)
    tones = ((1 << 62,), (0,), (a,))
    f = g.RfFrontend(tones=tones)
    got = f.run(np.ones(64, np.complex64))
    f.close()
    _within_tol(got, np.exp(1j * rr.phi(rr.params(tones=tones).tones, 0, 64)))


@pytest.mark.parametrize("first", [0, FAR])
def test_iq_and_dc_alone(g, random_x, first):
    mu, nu = g.RfFrontend.iq_imbalance(0.5, 3.0)
    for kw in (dict(mu=mu, nu=nu), dict(dc=0.25 - 0.5j), dict(mu=mu, nu=nu, dc=0.25 - 0.5j), dict(mu=0.5j), dict(nu=0.1)):
        f = g.RfFrontend(first_sample=first, **kw)
        got = f.run(random_x)
        f.close()
        _within_tol(got, rr.rf(random_x, rr.params(**kw), first))
        assert (got != random_x).mean() > 0.99


# ------------------------------------------------------------------ 3. everything at once
@pytest.fixture(scope="module")
def whole_runs(g, random_x):
    """first -> the one-call output of every stage on random_x, checked against the model once"""
    kw, p = _all_on(g)
    out = {}
    for first in (0, FAR):
        f = g.RfFrontend(first_sample=first, **kw)
        out[first] = f.run(random_x)
        f.close()
        _within_tol(out[first], rr.rf(random_x, p, first))
    return out


@pytest.mark.parametrize("first", [0, FAR])
def test_everything_at_once(g, random_x, whole_runs, first):
    assert (whole_runs[first] != whole_runs[FAR - first]).mean() > 0.999               # the position matters
    kw, _ = _all_on(g)
    kw["dc"] = 0                                                                       # and so does each stage
    f = g.RfFrontend(first_sample=first, **kw)
    assert (f.run(random_x) != whole_runs[first]).mean() > 0.999
    f.close()


# ------------------------------------------------------------------ 4. splits
SPLITS = [1, 2, 3, 61, 255, 256, 257, 1023, 1024, 1025]


def _cuts(n):
    sizes = SPLITS + [n - sum(SPLITS)]
    assert sizes[-1] > 0
    return sizes


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("first", [0, FAR])
def test_split_calls_equal_one_call_bit_for_bit(g, random_x, whole_runs, first, shift):
    x, whole = random_x, whole_runs[first]
    kw, _ = _all_on(g)
    f = g.RfFrontend(first_sample=first, **kw)
    # the device entry, cut; with shift = 1 the buffers begin 8 bytes behind a 16-byte boundary, so every piece's parity is the other one
    din, dout = Dev(g, n=N + 2), Dev(g, n=N + 2)
    din.put(x, at=shift)
    p = 0
    for n in _cuts(N):
        f.run_device(din.ptr + 8 * (shift + p), n, dout.ptr + 8 * (shift + p))
        p += n
    assert dout.get(shift, N).tobytes() == whole.tobytes()
    # after a reset: the same bytes again, in one device call, input and output of different parity
    f.reset()
    dout.put(np.zeros(N + 2, np.complex64))
    f.run_device(din.ptr + 8 * shift, N, dout.ptr + 8 * (1 - shift))
    assert dout.get(1 - shift, N).tobytes() == whole.tobytes()
    # in place, cut
    f.reset()
    p = 0
    for n in _cuts(N):
        f.run_device(din.ptr + 8 * (shift + p), n, din.ptr + 8 * (shift + p))
        p += n
    assert din.get(shift, N).tobytes() == whole.tobytes()
    # the host entry, cut (calls of 0 samples between)
    f.reset()
    parts, p = [], 0
    for n in _cuts(N):
        parts.append(f.run(x[p:p + n]))
        assert len(f.run(x[:0])) == 0 and len(parts[-1]) == n
        p += n
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    din.free(); dout.free(); f.close()


@pytest.mark.parametrize("first", [0, FAR])
def test_a_later_handle_continues_the_stream(g, random_x, whole_runs, first):
    s = 20001
    kw, _ = _all_on(g)
    f = g.RfFrontend(first_sample=first + s, **kw)
    tail = f.run(random_x[s:])
    f.close()
    assert tail.tobytes() == whole_runs[first][s:].tobytes()


# ------------------------------------------------------------------ 5. the two entries, two streams, refused calls
@pytest.mark.skipif(torch is None, reason="needs torch")
def test_device_entry_on_two_streams(g, random_x, whole_runs):
    kw, _ = _all_on(g)
    x1, x2 = random_x, random_x[::-1].copy()
    kw2 = dict(kw, tones=g.phase_noise_tones(MASK_20, 32, 6))
    r = g.RfFrontend(first_sample=FAR, **kw2)
    ref1, ref2 = whole_runs[0], r.run(x2)
    r.close()
    dev = torch.device("cuda:0")
    d1, d2 = torch.from_numpy(x1.view(np.float32).copy()).to(dev), torch.from_numpy(x2.view(np.float32).copy()).to(dev)
    o1 = torch.zeros_like(d1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = g.RfFrontend(**kw), g.RfFrontend(first_sample=FAR, **kw2)
    torch.cuda.synchronize()
    # two handles interleaved on two streams, each in three calls; handle a changes streams between its calls, handle b works in place
    cuts = [0, 9001, 9002, N]
    for i in range(3):
        lo, hi = cuts[i], cuts[i + 1]
        sa = s1 if i != 1 else s2
        a.run_device(d1.data_ptr() + 8 * lo, hi - lo, o1.data_ptr() + 8 * lo, stream=sa.cuda_stream)
        b.run_device(d2.data_ptr() + 8 * lo, hi - lo, d2.data_ptr() + 8 * lo, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert o1.cpu().numpy().view(np.complex64).tobytes() == ref1.tobytes()
    assert d2.cpu().numpy().view(np.complex64).tobytes() == ref2.tobytes()
    a.close(); b.close()


def test_refused_calls_leave_the_stream_intact(g, random_x, whole_runs):
    x = random_x[:20000]
    whole = whole_runs[0][:20000]
    kw, _ = _all_on(g)
    f = g.RfFrontend(**kw)
    L = g.lib()
    din, dout = Dev(g, x), Dev(g, n=len(x))
    f.run_device(din.ptr, 1001, dout.ptr)
    before = dout.get()
    run_device = L.dvbt_rf_run_device
    for inp, n, out in ((din.ptr + 8 * 1001, 100, din.ptr + 8 * 1011),            # the output begins inside the input
                        (din.ptr + 8 * 1001, 100, din.ptr + 8 * 902),             # the output ends inside the input
                        (din.ptr + 8 * 1001, 100, din.ptr + 8 * 1002),            # one sample off being in place
                        (din.ptr + 8 * 1001 + 4, 100, dout.ptr + 8 * 1001),       # a misaligned buffer
                        (din.ptr, 2 ** 31 + 1, dout.ptr),                         # more than a call takes (refused before anything is read)
                        (None, 100, dout.ptr + 8 * 1001),
                        (din.ptr + 8 * 1001, 100, None)):
        assert run_device(f.h, C.c_void_p(inp), n, C.c_void_p(out), None) == -1
    with pytest.raises(g.DvbtError):
        f.run_device(din.ptr + 8 * 1001, 100, din.ptr + 8 * 1011)
    assert din.get().tobytes() == x.tobytes() and dout.get().tobytes() == before.tobytes()
    f.run_device(din.ptr + 8 * 1001, len(x) - 1001, dout.ptr + 8 * 1001)           # continues where the last good call ended
    assert dout.get().tobytes() == whole.tobytes()
    din.free(); dout.free(); f.close()


# ------------------------------------------------------------------ 6. device-resident loopback
LOOPBACK = [(1, 0, 20.0, SEEDS[0], 6.0, MASK_20, 1.9, (0.5, 3.0)), (2, 4, 30.0, SEEDS[1], 10.0, MASK_30, 0.6, (0.2, 1.0))]


@pytest.mark.parametrize("const,cr,snr,seed,ibo,mask,rms,imb", LOOPBACK, ids=["2k_qam16_1_2_20dB", "2k_qam64_7_8_30dB"])
def test_loopback_that_never_leaves_the_device(g, po, const, cr, snr, seed, ibo, mask, rms, imb):
    """Tx -> RfFrontend(amplifier) -> Channel(noise) -> RfFrontend(tones, IQ imbalance, DC) -> Rx.  The chained models with these seeds, run through the
    oracle's receiver on the CPU (the oracle's modulator in the place of Tx), give one lock period and every delivered packet right: QAM16 1/2 with 0
    corrected RS symbols, QAM64 7/8 with 843 -- noise alone gives 0 in both, so the impairments are felt and the code has room."""
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
    meter = g.Channel()
    A = g.RfFrontend.saturation(ibo, meter.power(a.ptr + 8 * 1000, 100000))
    amp = g.RfFrontend(sat_amplitude=A, smoothness=2.0)
    amp.run_device(a.ptr, total, b.ptr)
    behind = meter.power(b.ptr + 8 * 1000, 100000)
    sigma = g.Channel.sigma(snr, behind)
    noisy = g.Channel(noise_sigma=sigma, seed=seed)
    noisy.run_device(b.ptr, total, y.ptr)
    noised = y.get()
    tones = g.phase_noise_tones(mask, 32, seed)                                    # the same seed: the table's counters are not the noise's
    assert abs(rr.rms_deg(tones) - rms) <= 0.06
    mu, nu = g.RfFrontend.iq_imbalance(*imb)
    dc = 0.05 * np.sqrt(behind) * np.exp(0.25j * np.pi)
    tuner = g.RfFrontend(tones=tones, mu=mu, nu=nu, dc=dc)
    tuner.run_device(y.ptr, total, y.ptr)                                          # in place
    rx = g.Rx(const, cr, mode, max_samples=total, snr_db=snr, taps=True)
    rep = rx.run_device(y.ptr, total)
    assert rep.n_lock_periods == 1
    got_ts = rx.tap(g.TAP_TS)
    p0 = rep.first_out_symbol * ibits // 8 // 204 + rep.ts_first_packet - 11
    n = len(got_ts) // 188
    assert n > 0 and p0 >= 0 and p0 + n <= npk
    assert (got_ts.reshape(-1, 188) == ts.reshape(-1, 188)[p0:p0 + n]).all()
    # the same samples on the host: what the three models chained say they are, and what the oracle's receiver makes of them
    host, amped = y.get(), b.get()
    model_amped = rr.rf(a.get(), rr.params(sat_amplitude=A))
    _within_tol(amped, model_amped)
    assert np.abs(amped).max() <= A * (1 + 2e-7)
    ref_power = np.mean(np.abs(amped[1000:101000].astype(np.complex128)) ** 2)
    assert abs(sigma - np.sqrt(ref_power / 10 ** (snr / 10) / 2)) <= 1e-6 * sigma
    model_noised = chanref.channel(model_amped, noise_sigma=sigma, seed=seed)
    _within_tol(noised, model_noised)
    _within_tol(host, rr.rf(model_noised, rr.params(tones=tones, mu=mu, nu=nu, dc=dc)))
    o = po.rx(c, host, snr_db=snr, want=INT_TAPS)
    assert o["truncated"] == 0 and rep.first_out_symbol == o["first_out_symbol"]
    for name in INT_TAPS:
        x, r = rx.tap(getattr(g, "TAP_" + {"vit": "VITERBI"}.get(name, name.upper()))), o[name]
        assert x.size == r.size > 0, name
        assert (x.reshape(-1) == r.reshape(-1)).all(), name
    assert rep.rs_fail_words == o["rs_fail"] and rep.rs_corrected_symbols == o["rs_corr"]
    print(f"\ncorrected RS symbols {rep.rs_corrected_symbols}, failed words {rep.rs_fail_words}")
    if const == 2:
        assert rep.rs_corrected_symbols > 0                                        # the impairments are felt
    rx.close(); tx.close(); amp.close(); meter.close(); noisy.close(); tuner.close()
    a.free(); b.free(); y.free(); L.dvbt_device_free(C.c_void_p(dts))
