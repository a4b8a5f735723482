"""The GPU tuner block (dvbt_tuner_*, gr_dvbt_amd.Tuner) against its numpy model tests/tunerref.py, the pinned resampler block and the receiver.

Without a shift the block is compared bit for bit with the float32 model: conversion, products and sums are single rounded float32 operations in a fixed
order on both sides.  With a shift the device's cosine and sine are a float polynomial, so the comparison is against the complex128 model within 1e-5 of
its peak sample, the project's bound for a float32 baseband (test_gpu_clock_block._within_tol).  What a stream looks like cut into calls, run through
the host or the device entry, run again after a reset or continued by a second handle is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import tunerref as tr

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FAR = 2 ** 40 + 3
N = 70000
FMT_IDS = ["cf32", "cs16", "cs8", "cu8"]


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
    """nbytes on the device (the library's own allocator and blocking copies: ordered with work on the default stream); x: any numpy array, as its bytes"""

    def __init__(self, g, x=None, nbytes=None):
        self.L = g.lib()
        self.nbytes = np.ascontiguousarray(x).nbytes if x is not None else nbytes
        self.ptr = self.L.dvbt_device_malloc(self.nbytes + 64)
        assert self.ptr
        self.put(np.zeros(self.nbytes, np.uint8) if x is None else x)

    def put(self, x, at=0):
        x = np.ascontiguousarray(x)
        if x.nbytes:
            assert self.L.dvbt_copy_to_device(C.c_void_p(self.ptr + at), x.ctypes.data_as(C.c_void_p), x.nbytes) == 0

    def get(self, at=0, nbytes=None, dtype=np.uint8):
        nbytes = self.nbytes - at if nbytes is None else nbytes
        out = np.zeros(nbytes, np.uint8)
        if nbytes:
            assert self.L.dvbt_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + at), nbytes) == 0
        return out.view(dtype)

    def samples(self, n, at=0):
        return self.get(8 * at, 8 * n, np.complex64)

    def free(self):
        self.L.dvbt_device_free(C.c_void_p(self.ptr))
        self.ptr = None


def _within_tol(got, model):
    assert got.shape == model.shape and got.dtype == np.complex64 and len(model) > 0
    assert np.isfinite(got.view(np.float32)).all()
    err, peak = np.abs(got - model).max(), np.abs(model).max()
    print(f"\nlargest error {err:.3e} = {err / peak:.2e} of the peak {peak:.4f}")
    assert err <= 1e-5 * peak


def _raw(fmt, n, seed=29):
    rng = np.random.RandomState(seed + fmt)
    if fmt == tr.CF32:
        x = (rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)
        if n:
            x[0] = complex(-0.0, 0.0)
        return x
    info = np.iinfo(tr.DTYPES[fmt])
    return rng.randint(info.min, info.max + 1, size=2 * n).astype(tr.DTYPES[fmt])


def _cut(raw, fmt, a, b):
    return raw[a:b] if fmt == tr.CF32 else raw[2 * a:2 * b]


@pytest.fixture(scope="module")
def raws():
    return [_raw(fmt, N) for fmt in range(4)]


@pytest.fixture(scope="module")
def model():
    """the float32 model of a no-shift configuration on the module's raw streams, computed once"""
    cache = {}

    def get(raws, fmt, L, M, swap=False):
        key = (fmt, L, M, swap)
        if key not in cache:
            cache[key] = tr.tuner(raws[fmt], fmt, L, M, swap_iq=swap)
            cache[key].flags.writeable = False
        return cache[key]
    return get


# ------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 4097])
def test_identity_is_bit_exact(g, raws, n):
    x = raws[tr.CF32][:n]
    t = g.Tuner(g.IQ_CF32, 1, 1, taps=[1.0], scale=1.0)
    assert t.outputs_for(n) == n and (t.desc.nt, t.desc.ntaps, t.delay) == (1, 1, 0)
    got = t.run(x)
    t.close()
    assert got.tobytes() == x.tobytes()                      # -0.0 at x[0] included


# ------------------------------------------------------------------ 2. no shift: the model's bits
CONFIGS = [(f, 32, 35) for f in range(4)] + [(tr.CS16, 8, 7), (tr.CS16, 16, 35), (tr.CS16, 1, 8), (tr.CS16, 128, 175)]


@pytest.mark.parametrize("swap", [False, True], ids=["iq", "qi"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{FMT_IDS[c[0]]}-{c[1]}/{c[2]}")
def test_without_a_shift_the_bits_are_the_models(g, raws, model, cfg, swap):
    fmt, L, M = cfg
    t = g.Tuner(fmt, 2 * L, 2 * M, swap_iq=swap)
    want_taps = tr.design(L, M)
    taps = t.taps
    assert len(taps) == len(want_taps) and np.abs(taps.astype(np.float64) - want_taps).max() <= 2.0 ** -22 * np.abs(want_taps).max()
    assert (t.desc.interpolation, t.desc.decimation, t.desc.nt) == (L, M, -(-len(taps) // L))
    assert t.delay * 2 * M == len(taps) - 1 and t.desc.phase_inc == 0
    got = t.run(raws[fmt] if fmt == tr.CF32 else raws[fmt].reshape(-1, 2))
    t.close()
    want = model(raws, fmt, L, M, swap) if taps.tobytes() == want_taps.tobytes() else tr.tuner(raws[fmt], fmt, L, M, taps=taps, swap_iq=swap)
    assert len(got) == len(want) == tr.outputs(N, L, M)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("fmt", [tr.CS16, tr.CU8], ids=["cs16", "cu8"])
def test_the_longest_prototype_and_the_widest_tile(g, raws, fmt):
    """25/199 with 8000 taps of the caller's: 320 taps per branch, 2350 staged samples a tile, 50.8 KB of LDS -- more than a launch gets without asking"""
    L, M = 25, 199
    taps = (np.random.RandomState(5).randn(8000) * np.hanning(8000)).astype(np.float32)
    t = g.Tuner(fmt, L, M, taps=taps)
    assert (t.desc.nt, t.desc.ntaps, t.delay * 2 * M) == (320, 8000, 7999) and t.taps.tobytes() == taps.tobytes()
    got = np.concatenate([t.run(_cut(raws[fmt], fmt, 0, 319)), t.run(_cut(raws[fmt], fmt, 319, N))])
    t.close()
    want = tr.tuner(raws[fmt], fmt, L, M, taps=taps)
    assert len(got) == len(want) == tr.outputs(N, L, M) > 8 * 256
    assert got.tobytes() == want.tobytes()


def test_a_dtype_that_is_not_the_formats_is_refused(g, raws):
    t = g.Tuner(g.IQ_CS16, 32, 35)
    for bad in (raws[tr.CF32][:10], raws[tr.CS8][:20], raws[tr.CU8][:20], np.zeros(20, np.float32), raws[tr.CS16][:21]):
        with pytest.raises(ValueError):
            t.run(bad)
    assert len(t.run(raws[tr.CS16][:70])) == 32
    t.close()


# ------------------------------------------------------------------ 3. the formats are one path
@pytest.mark.parametrize("fmt", [tr.CS16, tr.CS8, tr.CU8], ids=FMT_IDS[1:])
def test_an_integer_format_equals_cf32_fed_the_converted_samples(g, raws, fmt):
    scale = np.float32(tr.SCALES[fmt])
    i, q = tr.components(raws[fmt], fmt)
    off = np.float32(127.5 if fmt == tr.CU8 else 0.0)
    v = np.empty(N, np.complex64)
    v.real, v.imag = (i - off) * scale, (q - off) * scale
    a, b = g.Tuner(fmt, 32, 35), g.Tuner(g.IQ_CF32, 32, 35, scale=1.0)
    ya, yb = a.run(raws[fmt]), b.run(v)
    a.close(); b.close()
    assert len(ya) == tr.outputs(N, 32, 35) and ya.tobytes() == yb.tobytes()


# ------------------------------------------------------------------ 4. with a shift
@pytest.mark.parametrize("shift", [0.05, -0.25, 2.0 ** -40], ids=["0.05", "-0.25", "2^-40"])
@pytest.mark.parametrize("fmt,first_in", [(tr.CS16, 0), (tr.CF32, 0), (tr.CU8, FAR)], ids=["cs16", "cf32", "cu8-far"])
def test_with_a_shift_against_the_complex128_model(g, raws, fmt, first_in, shift):
    t = g.Tuner(fmt, 32, 35, shift=shift, first_in=first_in)
    assert t.desc.phase_inc == tr.increment(shift) != 0
    got = t.run(raws[fmt])
    taps = t.taps
    t.close()
    _within_tol(got, tr.tuner(raws[fmt], fmt, 32, 35, shift=shift, taps=taps, first_in=first_in, exact=True))


# ------------------------------------------------------------------ 5. splits
def _inputs_for_outputs(L, M, pos, want):
    """the fewest inputs behind stream position pos that complete `want` outputs"""
    n = want * M // L - 2
    while tr.outputs(pos + n, L, M) - tr.outputs(pos, L, M) < want:
        n += 1
    return n


def _sizes(L, M, nt, total, seed):
    """call sizes: 0, 1, 2, nt - 1, an odd count (the next call of a 2-byte format then begins on a 2-byte boundary), calls that emit 255 / 256 / 257 outputs
    and 20 random cuts of the rest"""
    sizes = [0, 1, 2, nt - 1, 3, 0, 1]                      # (the second call begins at sample 1: an odd sample)
    pos = sum(sizes)
    for want in (255, 256, 257):
        n = _inputs_for_outputs(L, M, pos, want)
        assert tr.outputs(pos + n, L, M) - tr.outputs(pos, L, M) in ((want,) if L <= M else (want, want + 1))      # (L > M: an input can complete two)
        sizes.append(n)
        pos += n
    cuts = np.sort(np.random.RandomState(seed).randint(pos, total, size=20))
    for c in list(cuts) + [total]:
        sizes.append(int(c) - pos)
        pos = int(c)
    assert sum(sizes) == total
    return sizes


SPLIT_CONFIGS = [(f, 32, 35, 0.0) for f in range(4)] + [(tr.CS16, 1, 8, 0.0), (tr.CS8, 8, 7, 0.05), (tr.CU8, 128, 175, -0.25)]


@pytest.mark.parametrize("cfg", SPLIT_CONFIGS, ids=lambda c: f"{FMT_IDS[c[0]]}-{c[1]}/{c[2]}-{c[3]}")
def test_split_calls_equal_one_call_bit_for_bit(g, raws, cfg):
    fmt, L, M, shift = cfg
    raw, bps = raws[fmt], tr.BYTES[fmt]
    t = g.Tuner(fmt, L, M, shift=shift)
    nt = t.desc.nt
    params = g.TunerParams.of(fmt, L, M, shift=shift)
    whole = t.run(raw)
    assert len(whole) == tr.outputs(N, L, M) == g.tuner_outputs(params, N)
    sizes = _sizes(L, M, nt, N, 7 + fmt)
    # the host entry, cut
    t.reset()
    parts, p = [], 0
    for n in sizes:
        want = t.outputs_for(n)
        assert want == tr.outputs(p + n, L, M) - tr.outputs(p, L, M)
        parts.append(t.run(_cut(raw, fmt, p, p + n)))
        assert len(parts[-1]) == want
        p += n
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    # the device entry, cut the same way, on the default stream: the pointers are aligned to one raw sample only
    t.reset()
    din, dout = Dev(g, raw), Dev(g, nbytes=8 * (len(whole) + 1))
    p = q = 0
    odd = 0
    for n in sizes:
        want = t.outputs_for(n)
        odd += (din.ptr + bps * p) % 16 != 0 and n > 0
        assert t.run_device(din.ptr + bps * p, n, dout.ptr + 8 * q, len(whole) + 1 - q) == want
        p += n
        q += want
    assert odd >= 10
    assert q == len(whole) and dout.samples(q).tobytes() == whole.tobytes()
    # after a reset: the same bytes again, in one device call
    t.reset()
    dout.put(np.zeros(8 * (len(whole) + 1), np.uint8))
    assert t.run_device(din.ptr, N, dout.ptr, len(whole)) == len(whole)
    assert dout.samples(len(whole)).tobytes() == whole.tobytes()
    din.free(); dout.free(); t.close()


def test_device_entry_on_two_streams(g, raws):
    n = 20000
    ka, kb = dict(format=tr.CS8, interpolation=32, decimation=35, shift=0.05), dict(format=tr.CS16, interpolation=16, decimation=35)
    x1, x2 = raws[tr.CS8][2 * 901:2 * (901 + n)], raws[tr.CS16][2 * 30000:2 * (30000 + n)]
    ra, rb = g.Tuner(**ka), g.Tuner(**kb)
    ref1, ref2 = ra.run(x1), rb.run(x2)
    ra.close(); rb.close()
    assert len(ref1) == tr.outputs(n, 32, 35) and len(ref2) == tr.outputs(n, 16, 35)
    dev = torch.device("cuda:0")
    d1, d2 = torch.from_numpy(x1.copy()).to(dev), torch.from_numpy(x2.copy()).to(dev)
    o1, o2 = torch.zeros(2 * len(ref1), dtype=torch.float32, device=dev), torch.zeros(2 * len(ref2), dtype=torch.float32, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = g.Tuner(**ka), g.Tuner(**kb)
    torch.cuda.synchronize()
    # two handles interleaved on two streams, each in three calls; handle a changes streams between its calls
    cuts = [0, 9001, 9002, n]
    qa = qb = 0
    for i in range(3):
        lo, hi = cuts[i], cuts[i + 1]
        sa = s1 if i != 1 else s2
        qa += a.run_device(d1.data_ptr() + 2 * lo, hi - lo, o1.data_ptr() + 8 * qa, len(ref1) - qa, stream=sa.cuda_stream)
        qb += b.run_device(d2.data_ptr() + 4 * lo, hi - lo, o2.data_ptr() + 8 * qb, len(ref2) - qb, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert qa == len(ref1) and qb == len(ref2)
    assert o1.cpu().numpy().view(np.complex64).tobytes() == ref1.tobytes()
    assert o2.cpu().numpy().view(np.complex64).tobytes() == ref2.tobytes()
    a.close(); b.close()


@pytest.mark.parametrize("cfg", [(tr.CS16, 32, 35, 0.05), (tr.CU8, 1, 8, 0.0), (tr.CF32, 8, 7, -0.25)], ids=lambda c: f"{FMT_IDS[c[0]]}-{c[1]}/{c[2]}")
def test_a_second_handle_continues_a_cut_stream(g, raws, cfg):
    fmt, L, M, shift = cfg
    raw = raws[fmt]
    n0 = 30001
    w = g.Tuner(fmt, L, M, shift=shift)
    whole = w.run(raw)
    ntaps = w.desc.ntaps
    w.close()
    ph = g.Tuner(fmt, L, M, shift=shift, first_in=n0)
    piece = ph.run(_cut(raw, fmt, n0, N))
    ph.close()
    ma, m1 = tr.total(n0, L, M), tr.first_whole_output(n0, ntaps, L, M)
    assert len(piece) == len(whole) - ma and m1 < len(whole) - 1000
    assert piece[m1 - ma:].tobytes() == whole[m1:].tobytes()


@pytest.mark.parametrize("cfg", CONFIGS[1:4] + CONFIGS[6:], ids=lambda c: f"{FMT_IDS[c[0]]}-{c[1]}/{c[2]}")
def test_far_into_a_stream(g, raws, cfg):
    fmt, L, M = cfg
    raw = _cut(raws[fmt], fmt, 1, 4098)
    t = g.Tuner(fmt, L, M, first_in=FAR)
    taps = t.taps
    got = np.concatenate([t.run(_cut(raw, fmt, 0, 1001)), t.run(_cut(raw, fmt, 1001, 4097))])
    t.close()
    assert len(got) == tr.outputs(4097, L, M, FAR) == g.tuner_outputs(g.TunerParams.of(fmt, L, M, first_in=FAR), 4097)
    assert got.tobytes() == tr.tuner(raw, fmt, L, M, taps=taps, first_in=FAR).tobytes()


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("fmt", [tr.CS16, tr.CS8], ids=["cs16", "cs8"])
def test_refused_calls_leave_the_stream_intact(g, raws, fmt):
    n_all, bps = 20000, tr.BYTES[fmt]
    raw = _cut(raws[fmt], fmt, 0, n_all)
    fresh = g.Tuner(fmt, 32, 35, shift=0.05)
    whole = fresh.run(raw)
    fresh.close()
    t = g.Tuner(fmt, 32, 35, shift=0.05)
    L = g.lib()
    din, dout = Dev(g, raw), Dev(g, nbytes=8 * n_all)
    n1 = t.run_device(din.ptr, 1001, dout.ptr, n_all)
    assert n1 == tr.outputs(1001, 32, 35)
    before = dout.get()
    rest = n_all - 1001
    want = t.outputs_for(rest)
    assert n1 + want == len(whole)
    run_device = L.dvbt_tuner_run_device
    nout = C.c_size_t(12345)
    inp, out = din.ptr + bps * 1001, dout.ptr + 8 * n1
    # one slot short
    assert run_device(t.h, C.c_void_p(inp), rest, C.c_void_p(out), want - 1, C.byref(nout), None) == -4   # DVBT_ERR_CAPACITY
    with pytest.raises(g.DvbtError):
        t.run_device(inp, rest, out, want - 1)
    room = Dev(g, nbytes=8 * 4096)                                     # a second buffer to overlap with: [input | output] and [output | input]
    for i, n, o in ((room.ptr, 1000, room.ptr + bps * 1000 - 8),       # the output begins inside the input's last bytes
                    (room.ptr, 1000, room.ptr),                        # in place
                    (room.ptr + 8 * 914 - bps, 1000, room.ptr),        # the output (914 samples) ends inside the input's first sample
                    (inp + bps // 2, 100, out),                        # an input misaligned by half a raw sample
                    (inp, 100, out + 4),                               # a misaligned output
                    (din.ptr, 2 ** 31 + 1, dout.ptr),                  # more than a call takes (refused before anything is read)
                    (None, 100, out),
                    (inp, 100, None)):
        assert run_device(t.h, C.c_void_p(i), n, C.c_void_p(o), n_all, C.byref(nout), None) == -1, (i, n, o)
    assert tr.outputs(1001 + 1000, 32, 35) - tr.outputs(1001, 32, 35) in (914, 915)
    assert t.outputs_for(rest) == want
    assert din.get().tobytes() == raw.view(np.uint8).tobytes() and dout.get().tobytes() == before.tobytes()
    assert not room.get().any()
    assert t.run_device(inp, rest, out, want) == want                  # continues where the last good call ended
    assert dout.samples(len(whole)).tobytes() == whole.tobytes()
    # the host entry refuses the same way and goes on as well
    t.reset()
    o = np.zeros(len(whole), np.complex64)
    z = C.c_size_t()
    assert L.dvbt_tuner_run(t.h, raw.ctypes.data_as(C.c_void_p), n_all, o.ctypes.data_as(C.c_void_p), len(whole) - 1, C.byref(z)) == -4
    assert not o.any()
    assert t.run(raw).tobytes() == whole.tobytes()
    din.free(); dout.free(); room.free(); t.close()


# ------------------------------------------------------------------ 7. against the pinned resampler block
def test_against_the_pinned_resampler(g, raws):
    n_in, scale = 50000, 0.00055242272
    x = raws[tr.CF32][:n_in]
    b = g.Block("resampler", 64, 70, scale)
    fn = b.L.dvbt_resampler_get_taps
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    ri, rd = C.c_int(), C.c_int()
    ntaps = fn(b.h, None, 0, C.byref(ri), C.byref(rd))
    taps = np.zeros(ntaps, np.float32)
    assert fn(b.h, taps.ctypes.data_as(C.c_void_p), ntaps, None, None) == ntaps and (ri.value, rd.value) == (32, 35)
    cap = tr.outputs(n_in, 32, 35) + 64
    ref = np.zeros(cap, np.complex64)
    produced, consumed, _ = b.work(cap, n_in, x.copy(), ref)
    b.close()
    t = g.Tuner(g.IQ_CF32, 64, 70, taps=taps, scale=scale)
    assert (t.desc.interpolation, t.desc.decimation, t.desc.ntaps) == (32, 35, ntaps) and t.taps.tobytes() == taps.tobytes()
    got = t.run(x)
    t.close()
    n = min(produced, len(got))
    assert n >= tr.outputs(n_in, 32, 35) - 40 and consumed >= n_in - 40
    _within_tol(got[:n], ref[:n].astype(np.complex128))
    print(f"the bits are equal too: {got[:n].tobytes() == ref[:n].tobytes()} (the block scales the sum, the tuner the samples)")
    t1 = g.Tuner(g.IQ_CF32, 64, 70, taps=taps, scale=1.0)
    b1 = g.Block("resampler", 64, 70, 1.0)
    ref1 = np.zeros(cap, np.complex64)
    p1, _, _ = b1.work(cap, n_in, x.copy(), ref1)
    got1 = t1.run(x)
    b1.close(); t1.close()
    n1 = min(p1, len(got1))
    print(f"with scale 1 on both: {got1[:n1].tobytes() == ref1[:n1].tobytes()}")


# ------------------------------------------------------------------ 8. through the receiver
@pytest.fixture(scope="module")
def capture(g, po):
    """the CPU test's construction (test_tuner_model) with the GPU tuner on both legs: (cfg, src, the int16 capture, the tuned baseband)"""
    c = po.cfg(po.QAM16, po.C1_2, po.T2k)
    src = po.stream_slice(c, 4, 13)
    up_h = g.Tuner(g.IQ_CF32, 35, 32)
    up = up_h.run(src)
    up_h.close()
    raw = tr.capture_cs16(up, 0.05)
    t = g.Tuner(g.IQ_CS16, 32, 35, shift=-0.05)
    iq = t.run(raw)
    t.close()
    assert len(iq) == tr.outputs(len(up), 32, 35) and abs(len(iq) - len(src)) <= 1
    return c, src, raw, iq


def test_the_receiver_decodes_the_tuned_capture(g, po, capture):
    c, src, raw, iq = capture
    o = po.rx(c, iq, snr_db=30, want=("ts",))
    assert not o["truncated"]
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
    ref = po.rx(c, src, snr_db=30, want=("ts",))["ts"]
    n = tr.ts_common_packets(ts, ref)
    print(f"\n{len(ts) // 188} packets from the tuned capture, {len(ref) // 188} from the original, {n} in common")
    assert n >= 2 * po.packets_per_superframe(c)


def test_feed_into_a_stream_equals_a_push_of_the_whole_output(g, capture):
    c, src, raw, iq = capture
    a = g.RxStream(g.QAM16, g.C1_2, g.T2k, segment_superframes=1)
    a.push(iq)
    a.finish()
    want = a.pull()
    a.close()
    b = g.RxStream(g.QAM16, g.C1_2, g.T2k, segment_superframes=1)
    t = g.Tuner(g.IQ_CS16, 32, 35, shift=-0.05)
    fed = 0
    for lo in range(0, len(raw) // 2, 100003):
        fed += t.feed(b, raw[2 * lo:2 * (lo + 100003)])
    t.close()
    b.finish()
    got = b.pull()
    b.close()
    assert fed == len(iq)
    assert len(want) > 0 and got.tobytes() == want.tobytes()
