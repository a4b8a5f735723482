"""The GPU sample-clock offset block (dvbt_clock_*, gr_dvbt_amd.ClockOffset) against its numpy model tests/clockref.py and the oracle's resampler
po.clock_offset.

TOL: 1e-5 of the model's peak sample, the project's bound for a float32 baseband (test_gpu_tx._close); the kernel's own error is a few 1e-7 (float32
coefficients and sums over 16 to 64 taps).  What a stream looks like cut into calls, run through the host or the device entry, run again after a reset or
continued by a second handle is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import clockref

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FAR = 2 ** 40 + 3


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
    assert np.isfinite(got.view(np.float32)).all()
    err, peak = np.abs(got - model).max(), np.abs(model).max()
    print(f"\nlargest error {err:.3e} = {err / peak:.2e} of the peak {peak:.4f}")
    assert err <= 1e-5 * peak


@pytest.fixture(scope="module")
def random_x():
    rng = np.random.RandomState(29)
    x = (rng.randn(300000) + 1j * rng.randn(300000)).astype(np.complex64)
    x[0] = complex(-0.0, 0.0)
    return x


# ------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 4097])
@pytest.mark.parametrize("start", [0, 5, None])
def test_identity_is_bit_exact(g, random_x, start, n):
    for taps in (16, 64):
        H = taps // 2
        s = H if start is None else start
        ck = g.ClockOffset(0.0, start=start, taps=taps)
        x = random_x[:n]
        assert ck.outputs_for(n) == max(0, n - H - s)
        got = ck.run(x)
        assert len(got) == max(0, n - H - s)
        assert got.tobytes() == x[s:s + len(got)].tobytes()           # -0.0 at x[0] included (start = 0)
        ck.close()


# ------------------------------------------------------------------ 2. against the model
@pytest.fixture(scope="module")
def model():
    cache = {}

    def get(x, ppm, taps):
        if (ppm, taps) not in cache:
            cache[(ppm, taps)] = clockref.resample(x, ppm, taps=taps)
        return cache[(ppm, taps)]
    return get


@pytest.mark.parametrize("ppm", [10.0, -40.0, 55.0, 1000.0, -1000.0])
@pytest.mark.parametrize("taps", [16, 32, 64])
def test_against_the_model_and_the_oracle(g, po, random_x, model, taps, ppm):
    x = random_x[:200000]
    ck = g.ClockOffset(ppm, taps=taps)
    got = ck.run(x)
    ck.close()
    _within_tol(got, model(x, ppm, taps))
    if taps == 16:
        ref = po.clock_offset(x, ppm)
        n = min(len(ref), len(got))
        assert n > 199000 / (1 + ppm * 1e-6)
        _within_tol(got[:n], ref[:n].astype(np.complex128))


# ------------------------------------------------------------------ 3. fractions
@pytest.mark.parametrize("frac", [2.0 ** -40, 2.0 ** -33, 0.5, 1 - 2.0 ** -40], ids=["2^-40", "2^-33", "1/2", "1-2^-40"])
@pytest.mark.parametrize("taps", [16, 32, 64])
def test_small_and_large_fractions(g, random_x, taps, frac):
    x = random_x[:4097]
    start = taps // 2 + frac
    assert clockref.pos(0, 0.0, start)[1] == int(frac * 2 ** 64) != 0
    ck = g.ClockOffset(0.0, start=start, taps=taps)
    got = ck.run(x)
    ck.close()
    _within_tol(got, clockref.resample(x, 0.0, start=start, taps=taps))


# ------------------------------------------------------------------ 4. splits
N_SPLIT = 2 ** 18 + 1
SPLITS = [1, 63, 1000, 0, 4097]


@pytest.mark.parametrize("taps,ppm", [(16, 55.0), (64, -1000.0), (16, -1000.0), (64, 55.0)])
def test_split_calls_equal_one_call_bit_for_bit(g, random_x, taps, ppm):
    x = random_x[:N_SPLIT]
    sizes = SPLITS + [N_SPLIT - sum(SPLITS)]
    H = taps // 2
    params = g.ClockParams(ppm, float(H), taps, 0, 0, 0)
    ck = g.ClockOffset(ppm, taps=taps)
    whole = ck.run(x)
    assert len(whole) == clockref.outputs(N_SPLIT, ppm, H, taps) == g.clock_outputs(params, N_SPLIT)
    # the host entry, cut
    ck.reset()
    parts, p = [], 0
    for n in sizes:
        want = ck.outputs_for(n)
        assert want == g.clock_outputs(params, p + n) - g.clock_outputs(params, p) == clockref.outputs(p + n, ppm, H, taps) - clockref.outputs(p, ppm, H, taps)
        parts.append(ck.run(x[p:p + n]))
        assert len(parts[-1]) == want
        p += n
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    # the device entry, cut the same way, on the default stream
    ck.reset()
    din, dout = Dev(g, x), Dev(g, n=len(whole) + 1)
    p, q = 0, 0
    for n in sizes:
        want = ck.outputs_for(n)
        assert ck.run_device(din.ptr + 8 * p, n, dout.ptr + 8 * q, len(whole) + 1 - q) == want
        p += n
        q += want
    assert q == len(whole) and dout.get(0, q).tobytes() == whole.tobytes()
    # after a reset: the same bytes again, in one device call
    ck.reset()
    dout.put(np.zeros(len(whole) + 1, np.complex64))
    assert ck.run_device(din.ptr, N_SPLIT, dout.ptr, len(whole)) == len(whole)
    assert dout.get(0, len(whole)).tobytes() == whole.tobytes()
    din.free(); dout.free(); ck.close()


def test_device_entry_on_two_streams(g, random_x):
    N = 20000
    pa, pb = dict(taps=16, ppm=55.0), dict(taps=64, ppm=-1000.0)
    x1, x2 = random_x[900:900 + N], random_x[30000:30000 + N]
    ra, rb = g.ClockOffset(**pa), g.ClockOffset(**pb)
    ref1, ref2 = ra.run(x1), rb.run(x2)
    ra.close(); rb.close()
    assert len(ref1) > N - 100 and len(ref2) > N - 100
    dev = torch.device("cuda:0")
    d1, d2 = torch.from_numpy(x1.view(np.float32).copy()).to(dev), torch.from_numpy(x2.view(np.float32).copy()).to(dev)
    o1, o2 = torch.zeros(2 * len(ref1), dtype=torch.float32, device=dev), torch.zeros(2 * len(ref2), dtype=torch.float32, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = g.ClockOffset(**pa), g.ClockOffset(**pb)
    torch.cuda.synchronize()
    # two handles interleaved on two streams, each in three calls; handle a changes streams between its calls
    cuts = [0, 9001, 9002, N]
    qa = qb = 0
    for i in range(3):
        lo, hi = cuts[i], cuts[i + 1]
        sa = s1 if i != 1 else s2
        qa += a.run_device(d1.data_ptr() + 8 * lo, hi - lo, o1.data_ptr() + 8 * qa, len(ref1) - qa, stream=sa.cuda_stream)
        qb += b.run_device(d2.data_ptr() + 8 * lo, hi - lo, o2.data_ptr() + 8 * qb, len(ref2) - qb, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert qa == len(ref1) and qb == len(ref2)
    assert o1.cpu().numpy().view(np.complex64).tobytes() == ref1.tobytes()
    assert o2.cpu().numpy().view(np.complex64).tobytes() == ref2.tobytes()
    a.close(); b.close()


# ------------------------------------------------------------------ 5. far out, and pieces
@pytest.mark.parametrize("taps", [16, 64])
def test_far_into_a_stream(g, random_x, taps):
    x = random_x[1:4098]
    H, ppm = taps // 2, 37.5
    first_in = clockref.first_in_for(FAR, ppm, H, taps)
    ck = g.ClockOffset(ppm, taps=taps, first_out=FAR, first_in=first_in)
    got = ck.run(x)
    ck.close()
    assert len(got) == clockref.outputs(len(x), ppm, H, taps, FAR, first_in) > 4000 - taps
    _within_tol(got, clockref.resample(x, ppm, taps=taps, first_out=FAR, first_in=first_in))


@pytest.mark.parametrize("taps,ppm", [(16, 55.0), (64, -1000.0)])
def test_a_second_handle_continues_a_cut_stream(g, random_x, taps, ppm):
    x = random_x
    M = 100001
    whole_h = g.ClockOffset(ppm, taps=taps)
    whole = whole_h.run(x)
    whole_h.close()
    first_in = clockref.first_in_for(M, ppm, taps // 2, taps)
    piece_h = g.ClockOffset(ppm, taps=taps, first_out=M, first_in=first_in)
    piece = piece_h.run(x[first_in:])
    piece_h.close()
    assert len(piece) == len(whole) - M and piece.tobytes() == whole[M:].tobytes()


# ------------------------------------------------------------------ 6. refusals
def test_refused_calls_leave_the_stream_intact(g, random_x):
    x = random_x[:20000]
    ppm = 55.0
    fresh = g.ClockOffset(ppm)
    whole = fresh.run(x)
    fresh.close()
    ck = g.ClockOffset(ppm)
    L = g.lib()
    din, dout = Dev(g, x), Dev(g, n=len(x))
    n1 = ck.run_device(din.ptr, 1001, dout.ptr, len(x))
    assert n1 == clockref.outputs(1001, ppm, 8.0)
    before = dout.get()
    rest = len(x) - 1001
    want = ck.outputs_for(rest)
    assert n1 + want == len(whole)
    run_device = L.dvbt_clock_run_device
    nout = C.c_size_t(12345)
    # one slot short
    assert run_device(ck.h, C.c_void_p(din.ptr + 8 * 1001), rest, C.c_void_p(dout.ptr + 8 * n1), want - 1, C.byref(nout), None) == -4   # DVBT_ERR_CAPACITY
    with pytest.raises(g.DvbtError):
        ck.run_device(din.ptr + 8 * 1001, rest, dout.ptr + 8 * n1, want - 1)
    for inp, n, out in ((din.ptr + 8 * 1001, 100, din.ptr + 8 * 1011),            # the output begins inside the input
                        (din.ptr + 8 * 1001, 100, din.ptr + 8 * 1001),            # in place
                        (din.ptr + 8 * 1001, 100, din.ptr + 8 * 1000 - 8 * 50),   # the output ends inside the input
                        (din.ptr + 8 * 1001 + 4, 100, dout.ptr + 8 * n1),         # a misaligned input
                        (din.ptr + 8 * 1001, 100, dout.ptr + 8 * n1 + 4),         # a misaligned output
                        (din.ptr, 2 ** 31 + 1, dout.ptr),                         # more than a call takes (refused before anything is read)
                        (None, 100, dout.ptr + 8 * n1)):
        assert run_device(ck.h, C.c_void_p(inp), n, C.c_void_p(out), len(x), C.byref(nout), None) == -1
    assert ck.outputs_for(rest) == want
    assert din.get().tobytes() == x.tobytes() and dout.get().tobytes() == before.tobytes()
    assert ck.run_device(din.ptr + 8 * 1001, rest, dout.ptr + 8 * n1, want) == want     # continues where the last good call ended
    assert dout.get(0, len(whole)).tobytes() == whole.tobytes()
    din.free(); dout.free(); ck.close()


# ------------------------------------------------------------------ 7. through the receiver
@pytest.mark.parametrize("nsf,ppm", [(4, -40.0), (3, 55.0)])
def test_the_receiver_follows_the_blocks_offset(g, po, nsf, ppm):
    c = po.cfg(po.QAM16, po.C1_2, po.T2k)
    src = po.stream_slice(c, nsf, 13)
    cap = clockref.outputs(len(src), ppm, 8.0)                       # (more than len(src) where ppm < 0)
    din, dout = Dev(g, src), Dev(g, n=cap)
    ck = g.ClockOffset(ppm)
    n = ck.run_device(din.ptr, len(src), dout.ptr, cap)
    iq = dout.get(0, n)
    ck.close(); din.free(); dout.free()
    assert n == cap
    o = po.rx(c, iq, snr_db=30, want=("ts",))
    assert not o["truncated"]
    travel = int(o["cp_start"].max()) - int(o["cp_start"].min())
    assert travel > 64, travel
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=len(iq), snr_db=30)
    rep = rx.run(iq)
    cps = rx.tap(g.TAP_CP_START)
    ts = rx.tap(g.TAP_TS)
    rx.close()
    # (a lock that slips within the first calls makes the segment restart behind it: test_gpu_drift.py)
    skipped = o["n_acquired"] - rep.n_symbols
    assert 0 <= skipped <= 2 and (skipped == 0) == (rep.segment_offset == 0)
    assert (cps == o["cp_start"][skipped:]).all()
    assert rep.first_out_symbol == o["first_out_symbol"] - skipped >= 0
    assert len(ts) == len(o["ts"]) > 0 and (ts == o["ts"]).all()
