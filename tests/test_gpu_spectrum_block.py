"""The GPU spectrum analyser (dvbt_spectrum_*, gr_dvbt_amd.Spectrum) against its numpy model tests/specref.py.

The PSD's bound follows from the project's FFT bound: test_gpu_fft_sizes holds a transform's amplitudes to 1e-5 of its peak, so a bin's power is off by at
most 2e-5 sqrt(P Pmax) (Pmax: the model's largest single-segment bin, |X|^2 / (N sum w^2)), plus 1e-10 Pmax where P is next to nothing, plus 1e-6 P for the
float sums of 32 segments.  The histogram, the counts and the peak are integers and compared exactly; sum_power to 1e-6.  What a stream looks like cut into
calls, shifted by a sample in memory, through the host or the device entry, after a reset, across a read or on two streams is compared bit for bit: the
PSD's doubles, the histogram, every field.
"""
import ctypes as C

import numpy as np
import pytest

import specref as sr

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FS = sr.SAMPLE_RATE
HB = 1705 * FS / 2048 / 2
SEGMENT_COUNTS = (0, 1, 31, 32, 33, 67)
WINDOWS = {sr.RECT: "rect", sr.HANN: "hann", sr.BH4: "blackman-harris"}


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
        if x is not None:
            self.put(x)

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


def _bits(r):
    """the whole result, as bytes"""
    return (r.psd.tobytes(), r.hist.tobytes(), r.segments, r.samples_pushed, r.samples_counted, r.nonfinite, np.float64(r.sum_power).tobytes(),
            np.float32(r.peak_power).tobytes())


def _length(N, hop, S, extra=None):
    """samples that hold S complete segments and `extra` more (fewer than a further segment needs)"""
    extra = hop - 1 if extra is None else extra
    return N - 1 if S == 0 else N + (S - 1) * hop + extra


def _gauss(n, seed):
    rng = np.random.RandomState(seed)
    return ((rng.randn(n) + 1j * rng.randn(n)) * 0.25).astype(np.complex64)


def _two_tones(n, N):
    """two on-bin tones 80 dB apart, at +N/8 + 3 and -N/4 + 1 bins"""
    t = np.arange(n)
    return (np.exp(2j * np.pi * (N // 8 + 3) * t / N) + 1e-4 * np.exp(2j * np.pi * (1 - N // 4) * t / N)).astype(np.complex64)


def _check_against_model(got, want, what):
    """the PSD within the bound; the statistics exact (sum_power to 1e-6); returns the worst ratio to the bound"""
    assert (got.segments, got.samples_pushed, got.samples_counted, got.nonfinite) == (want.segments, want.samples_pushed, want.samples_counted, want.nonfinite), what
    assert np.array_equal(got.hist, want.hist), what
    assert np.float32(got.peak_power).tobytes() == np.float32(want.peak_power).tobytes(), what
    if want.nonfinite:
        assert np.isnan(got.sum_power) == np.isnan(want.sum_power) and np.isinf(got.sum_power) == np.isinf(want.sum_power), what
        return 0.0
    assert abs(got.sum_power - want.sum_power) <= 1e-6 * want.sum_power, what
    if want.segments == 0:
        assert not got.psd.any(), what
        return 0.0
    bound = 2e-5 * np.sqrt(want.psd * want.pmax) + 1e-10 * want.pmax + 1e-6 * want.psd
    ratio = float((np.abs(got.psd - want.psd) / bound).max())
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ------------------------------------------------------------------ 1. the PSD and the statistics against the model
@pytest.mark.parametrize("hop_of", ["N", "N/2", "N/8", "3N/8"])
@pytest.mark.parametrize("N", [64, 128, 2048, 8192])
def test_psd_and_statistics_against_the_model(g, N, hop_of):
    hop = {"N": N, "N/2": N // 2, "N/8": N // 8, "3N/8": 3 * N // 8}[hop_of]
    longest = _length(N, hop, max(SEGMENT_COUNTS))
    inputs = {"noise": _gauss(longest, N + hop), "two tones": _two_tones(longest, N)}
    worst = 0.0
    for kind, name in WINDOWS.items():
        s = g.Spectrum(N, hop if hop_of != "N/2" else None, name)              # None: the default, N / 2
        for S in SEGMENT_COUNTS:
            for what, x in inputs.items():
                x = x[:_length(N, hop, S)]
                s.reset()
                s.push(x)
                got = s.read()
                assert got.hop == hop and got.fft_size == N and got.window == kind
                worst = max(worst, _check_against_model(got, sr.welch(x, N, hop, kind), (N, hop, name, S, what)))
        s.close()
    print(f"\nN = {N}, hop = {hop}: worst |psd - model| / bound = {worst:.3f}")


def test_an_on_bin_tone_reads_its_power_over_the_enbw(g):
    N, A, b0 = 2048, 0.5, -300
    x = (A * np.exp(2j * np.pi * b0 * np.arange(40 * N) / N)).astype(np.complex64)
    for name in WINDOWS.values():
        s = g.Spectrum(N, window=name)
        s.push(x)
        r = s.read()
        s.close()
        assert int(np.argmax(r.psd)) == N // 2 + b0
        assert r.psd[N // 2 + b0] == pytest.approx(A * A / r.enbw, rel=1e-4)
        assert r.mean_power == pytest.approx(A * A, rel=1e-6) and r.freqs()[N // 2 + b0] == b0 * FS / N


def test_inf_and_nan_inside_the_counted_range(g):
    N, hop = 128, 48
    x = _gauss(_length(N, hop, 40), 77)
    x[100] = complex(np.inf, 1.0)
    x[1500] = complex(np.nan, 0.5)
    x[-1] = complex(np.inf, np.inf)                # behind the counted range
    s = g.Spectrum(N, hop, "hann")
    s.push(x)
    got = s.read()
    s.close()
    want = sr.welch(x, N, hop, sr.HANN)
    assert want.nonfinite == 2 and int(want.hist[2040]) == 1 and int(want.hist[2044]) == 1
    _check_against_model(got, want, "inf and nan")
    assert np.isnan(got.sum_power) and np.isnan(np.float32(got.peak_power))


# ------------------------------------------------------------------ 2. bit identity
def _one_call(g, x, N, hop, name):
    s = g.Spectrum(N, hop, name)
    s.push(x)
    r = s.read()
    s.close()
    return r


def _push_cut(push, x, sizes):
    p = 0
    for n in sizes:
        push(p, n)
        p += n
    assert p == len(x)


def _sizes(total, step):
    return [step] * (total // step) + ([total % step] if total % step else [])


def test_one_sample_calls(g):
    N, hop = 64, 24
    x = _gauss(_length(N, hop, 67, 5), 5)
    whole = _one_call(g, x, N, hop, "hann")
    assert whole.segments == 67
    _check_against_model(whole, sr.welch(x, N, hop, sr.HANN), "one call")
    d = Dev(g, x)
    s = g.Spectrum(N, hop, "hann")
    _push_cut(lambda p, n: s.push_device(d.ptr + 8 * p, n), x, [1] * len(x))
    assert _bits(s.read()) == _bits(whole)
    s.reset()
    _push_cut(lambda p, n: s.push(x[p:p + n]), x, [1] * len(x))                  # and the host entry
    assert _bits(s.read()) == _bits(whole)
    s.close(); d.free()


@pytest.fixture(scope="module")
def stream2k(g):
    """(x, N, hop, the one-call reading): 70 segments of 2048 at a hop of 768, so that groups end at segments 32 and 64"""
    N, hop = 2048, 768
    x = _gauss(_length(N, hop, 70, 100), 6)
    whole = _one_call(g, x, N, hop, "blackman-harris")
    assert whole.segments == 70
    _check_against_model(whole, sr.welch(x, N, hop, sr.BH4), "one call")
    return x, N, hop, whole


def _cuts_of(name, n, N, hop):
    edge = N + 31 * hop                            # the sample count that completes segment 31, the last of group 0
    return {"N-1": _sizes(n, N - 1), "hop": _sizes(n, hop), "prime": _sizes(n, 4099), "short of hop": _sizes(n, hop - 1),
            "at a group boundary": [edge, n - edge], "one before": [edge - 1, n - edge + 1], "one behind": [edge + 1, n - edge - 1],
            "both boundaries": [edge, 32 * hop, n - edge - 32 * hop], "one sample across": [edge - 1, 1, 1, n - edge - 1]}[name]


@pytest.mark.parametrize("cut", ["N-1", "hop", "prime", "short of hop", "at a group boundary", "one before", "one behind", "both boundaries", "one sample across"])
def test_split_calls_equal_one_call_bit_for_bit(g, stream2k, cut):
    x, N, hop, whole = stream2k
    sizes = _cuts_of(cut, len(x), N, hop)
    s = g.Spectrum(N, hop, "blackman-harris")
    d = Dev(g, n=len(x) + 1)
    for shift in (0, 1):                           # with shift = 1 the input begins 8 bytes behind a 16-byte boundary
        d.put(x, at=shift)
        s.reset()
        _push_cut(lambda p, n: s.push_device(d.ptr + 8 * (shift + p), n), x, sizes)
        s.push_device(d.ptr, 0)
        assert _bits(s.read()) == _bits(whole), shift
    s.reset()                                      # the host entry, with calls of 0 samples between
    _push_cut(lambda p, n: (s.push(x[p:p + n]), s.push(x[:0])), x, sizes)
    assert _bits(s.read()) == _bits(whole)
    s.close(); d.free()


def test_read_does_not_disturb_and_reset_starts_again(g, stream2k):
    x, N, hop, whole = stream2k
    s = g.Spectrum(N, hop, "blackman-harris")
    first = s.read()                               # nothing pushed yet
    assert (first.segments, first.samples_pushed, first.samples_counted, first.sum_power, float(first.peak_power)) == (0, 0, 0, 0.0, 0.0)
    assert not first.psd.any() and not first.hist.any()
    cut = N + 40 * hop + 17                        # inside group 1
    s.push(x[:cut])
    part = s.read()
    assert _bits(part) == _bits(s.read())          # a read repeated
    assert _bits(part) == _bits(_one_call(g, x[:cut], N, hop, "blackman-harris"))
    s.push(x[cut:])
    assert _bits(s.read()) == _bits(whole)         # read, then continue: the uninterrupted run
    s.reset()
    assert _bits(s.read()) == _bits(first)
    s.push(x)
    assert _bits(s.read()) == _bits(whole)
    s.close()


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_two_handles_on_two_streams_and_one_handle_on_two(g, stream2k):
    x, N, hop, whole = stream2k
    x2 = x[::-1].copy()
    whole2 = _one_call(g, x2, N, hop, "hann")
    dev = torch.device("cuda:0")
    d1, d2 = torch.from_numpy(x.view(np.float32).copy()).to(dev), torch.from_numpy(x2.view(np.float32).copy()).to(dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b, c = g.Spectrum(N, hop, "blackman-harris"), g.Spectrum(N, hop, "hann"), g.Spectrum(N, hop, "blackman-harris")
    torch.cuda.synchronize()
    cuts = [0, 9001, 9002, 30000, len(x)]
    for i in range(4):
        lo, hi = cuts[i], cuts[i + 1]
        a.push_device(d1.data_ptr() + 8 * lo, hi - lo, stream=s1.cuda_stream)
        b.push_device(d2.data_ptr() + 8 * lo, hi - lo, stream=s2.cuda_stream)
        c.push_device(d1.data_ptr() + 8 * lo, hi - lo, stream=(s1, s2)[i & 1].cuda_stream)     # one handle, two streams alternately
    ra, rb, rc = a.read(), b.read(), c.read()      # read synchronises with whatever stream pushed last
    assert _bits(ra) == _bits(whole) and _bits(rb) == _bits(whole2) and _bits(rc) == _bits(whole)
    torch.cuda.synchronize()
    a.close(); b.close(); c.close()


def test_refused_calls_leave_the_state_intact(g, stream2k):
    x, N, hop, whole = stream2k
    s = g.Spectrum(N, hop, "blackman-harris")
    d = Dev(g, x)
    s.push_device(d.ptr, 5000)
    push = g.lib().dvbt_spectrum_push_device
    for ptr, n in ((d.ptr + 8 * 5000 + 4, 100), (None, 100), (d.ptr, 2 ** 31 + 1)):
        assert push(s.h, C.c_void_p(ptr), n, None) == -1
    with pytest.raises(g.DvbtError):
        s.push_device(d.ptr + 4, 100)
    s.push_device(d.ptr + 8 * 5000, len(x) - 5000)
    assert _bits(s.read()) == _bits(whole)
    s.close(); d.free()


# ------------------------------------------------------------------ 3. on the device end to end: an amplifier's spectral regrowth
def test_shoulders_behind_the_amplifier_on_the_device(g, po):
    """Tx -> RfFrontend (amplifier at none, 9, 6, 3 dB of back-off) -> Spectrum, nothing leaving the device but the readings; the model runs on the same
    GPU output copied to the host."""
    c = po.cfg(po.QAM16, po.C1_2, po.T2k)
    npk = po.packets_per_superframe(c)
    ts = po.stream_ts(c, 0, 1, 7)
    L = g.lib()
    tx = g.Tx(g.QAM16, g.C1_2, g.T2k, scale=po.tx_scale(c), max_packets=npk)
    nbody = tx.samples_for(npk)
    dts = L.dvbt_device_malloc(len(ts) + 64)
    assert L.dvbt_copy_to_device(C.c_void_p(dts), ts.ctypes.data_as(C.c_void_p), len(ts)) == 0
    a, b = Dev(g, n=nbody), Dev(g, n=nbody)
    assert tx.run_device(dts, npk, a.ptr, nbody) == nbody
    skip = 20 * (c.N + c.cp)                                                   # the start transient
    n = nbody - skip
    N, hop = 1024, 512
    spec = g.Spectrum(N, hop, "hann")
    spec.push_device(a.ptr + 8 * skip, n)
    clean = spec.read()
    model = sr.welch(a.get(skip, n), N, hop, sr.HANN)
    _check_against_model(clean, model, "no amplifier")
    assert abs(clean.papr_db() - model.papr_db()) <= 1e-5 and clean.occupied_bandwidth(0.99) == model.occupied_bandwidth(0.99) <= 1705 * FS / 2048
    assert abs(clean.papr_db(1e-3) - model.papr_db(1e-3)) <= 1e-5                   # the histograms are equal; the mean powers to 1e-6
    shoulders = [clean.shoulder_db(HB)]
    worst = max(abs(p - q) for p, q in zip(shoulders[0], model.shoulder_db(HB)))
    for ibo in (9.0, 6.0, 3.0):
        amp = g.RfFrontend(sat_amplitude=g.RfFrontend.saturation(ibo, clean.mean_power), smoothness=2.0)
        amp.run_device(a.ptr, nbody, b.ptr)
        spec.reset()
        spec.push_device(b.ptr + 8 * skip, n)
        r = spec.read()
        m = sr.welch(b.get(skip, n), N, hop, sr.HANN)
        _check_against_model(r, m, ibo)
        shoulders.append(r.shoulder_db(HB))
        worst = max([worst] + [abs(p - q) for p, q in zip(shoulders[-1], m.shoulder_db(HB))])
        amp.close()
    print("\nshoulders (lower, upper) at none, 9, 6, 3 dB of back-off:", [(round(p, 2), round(q, 2)) for p, q in shoulders],
          f"largest difference to the model {worst:.2e} dB; PAPR {clean.papr_db():.2f} dB, 99 % bandwidth {clean.occupied_bandwidth(0.99) / 1e6:.3f} MHz")
    assert worst <= 0.05
    for side in (0, 1):
        v = [sh[side] for sh in shoulders]
        assert v[0] > v[1] > v[2] > v[3] and all(v[i] - v[i + 1] > 1.0 for i in range(3))
    spec.close(); tx.close(); a.free(); b.free(); L.dvbt_device_free(C.c_void_p(dts))
