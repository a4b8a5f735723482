"""The tuner block's specification on the CPU (tests/tunerref.py): the designed prototype meets its own figures at every supported ratio and attenuation,
the model's counts, cut streams and conversions are what the header says, a tone at the capture's offset lands at 0 Hz, and a stream that went through a
capture (up to 35/32, moved, quantised to int16) and back through the model tuner decodes in the oracle to the transport stream of the original."""
import math

import numpy as np
import pytest

import tunerref as tr

ATTENS = [50.0, 60.0, 70.0, 80.0, 90.0]
RATIOS = [(32, 35), (8, 7), (16, 35), (4, 7), (1, 8), (128, 175), (64, 175), (25, 28), (4, 5), (24, 35), (1, 2), (6, 7)]


# ------------------------------------------------------------------ the designed prototype
def _figures(L, M, atten):
    """(ripple, stopband) in dB relative to DC, float64, on >= 12,000 frequencies: the stop band on an FFT grid 32 times finer than 1 / ntaps (all of it, up to
    half the prototype's rate: whatever is there folds into the output), the pass band on 2,001 points of its own"""
    h = tr.design(L, M, atten_db=atten).astype(np.float64)
    stop = min(tr.STOP_EDGE, M / L - tr.PASS_EDGE) if L > M else tr.STOP_EDGE
    fp, fs = tr.PASS_EDGE / M, stop / M
    nfft = 1 << max(16, int(math.ceil(math.log2(32 * len(h)))))
    H = np.abs(np.fft.rfft(h, nfft)) / L
    f = np.arange(len(H)) / nfft
    sb = H[f >= fs]
    pb = tr.response_db(h, np.linspace(0.0, fp, 2001), L)
    assert len(sb) + len(pb) >= 12000
    return float(np.abs(pb).max()), float(20.0 * np.log10(sb.max()))


@pytest.mark.parametrize("atten", ATTENS)
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}/{r[1]}")
def test_the_designed_prototype_meets_its_figures(ratio, atten):
    L, M = ratio
    ripple, stop = _figures(L, M, atten)
    print(f"\n{L}/{M} at {atten:.0f} dB: ripple {ripple:.4f} dB, stop band {stop:.2f} dB")
    assert ripple <= 0.06
    assert stop <= -(atten - 1.0)


def test_the_prototype_is_odd_symmetric_and_sums_to_L():
    for L, M in RATIOS:
        h = tr.design(2 * L, 2 * M)
        assert len(h) % 2 == 1 and (h == h[::-1]).all() and h.dtype == np.float32
        assert abs(float(h.astype(np.float64).sum()) - L) < 1e-4 * L
        assert -(-len(h) // L) <= tr.MAX_NT and L * -(-len(h) // L) <= tr.MAX_BRANCH_FLOATS
    assert len(tr.design(32, 35, atten_db=45.0)) < len(tr.design(32, 35, atten_db=55.0))      # Kaiser's other formula below 50 dB


# ------------------------------------------------------------------ the model
def _raw(fmt, n, seed=3):
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


@pytest.mark.parametrize("ratio", [(32, 35), (8, 7), (1, 8), (128, 175)], ids=lambda r: f"{r[0]}/{r[1]}")
@pytest.mark.parametrize("fmt", range(4), ids=["cf32", "cs16", "cs8", "cu8"])
def test_model_counts_and_cut_streams(fmt, ratio):
    L, M = ratio
    N = 9001
    raw = _raw(fmt, N)
    taps = tr.design(L, M)
    nt = -(-len(taps) // L)
    for first_in, shift in ((0, 0.0), (2 ** 40 + 3, -0.05)):
        whole = tr.tuner(raw, fmt, L, M, shift=shift, taps=taps, first_in=first_in)
        assert len(whole) == tr.outputs(N, L, M, first_in) == -(-(first_in + N) * L // M) - -(-first_in * L // M)
        st = tr.Stream(fmt, L, M, shift=shift, taps=taps, first_in=first_in)
        cuts = [0, 0, 1, 3, nt + 1, 2 * nt, 2 * nt + 1, 4000, N]
        parts = []
        for a, b in zip(cuts, cuts[1:]):
            parts.append(st.run(_cut(raw, fmt, a, b)))
            assert len(parts[-1]) == tr.outputs(b, L, M, first_in) - tr.outputs(a, L, M, first_in)
        assert np.concatenate(parts).tobytes() == whole.tobytes()
    # a stream that begins at n0 equals the whole one from the stated output on
    whole = tr.tuner(raw, fmt, L, M, shift=0.05, taps=taps)
    n0 = 1234
    piece = tr.tuner(_cut(raw, fmt, n0, N), fmt, L, M, shift=0.05, taps=taps, first_in=n0)
    m1, ma = tr.first_whole_output(n0, len(taps), L, M), tr.total(n0, L, M)
    assert len(piece) == len(whole) - ma and m1 < len(whole)
    assert piece[m1 - ma:].tobytes() == whole[m1:].tobytes()
    if fmt == tr.CF32:
        assert piece[:m1 - ma].tobytes() != whole[ma:m1].tobytes()       # ... and not before: the history is missing there


def test_identity_keeps_the_bits():
    x = _raw(tr.CF32, 300)
    y = tr.tuner(x, tr.CF32, 1, 1, taps=[1.0])
    assert y.tobytes() == x.tobytes() and np.signbit(y[0].real) and not np.signbit(y[0].imag)
    swapped = np.empty_like(x)
    swapped.real, swapped.imag = x.imag, x.real
    assert tr.tuner(x, tr.CF32, 3, 3, taps=[1.0], swap_iq=True).tobytes() == swapped.tobytes()


@pytest.mark.parametrize("fmt", [tr.CS16, tr.CS8, tr.CU8], ids=["cs16", "cs8", "cu8"])
def test_every_raw_value_converts_to_the_stated_float(fmt):
    info = np.iinfo(tr.DTYPES[fmt])
    vals = np.arange(info.min, info.max + 1, dtype=np.int64)
    raw = np.empty(2 * len(vals), tr.DTYPES[fmt])
    raw[0::2], raw[1::2] = vals, vals[::-1]
    off = 127.5 if fmt == tr.CU8 else 0.0
    for scale in (None, 1.0, 3.0e-5, -0.7):
        s = np.float64(np.float32(tr.SCALES[fmt] if scale is None else scale))
        # raw - 127.5 is exact in float32, and the float64 product of two float32 is exact: its rounding is the one rounded float32 multiply
        want_i, want_q = ((vals - off) * s).astype(np.float32), ((vals[::-1] - off) * s).astype(np.float32)
        got = tr.convert(raw, fmt, scale)
        assert got.real.tobytes() == want_i.tobytes() and got.imag.tobytes() == want_q.tobytes()
        got = tr.convert(raw.reshape(-1, 2), fmt, scale, swap_iq=True)
        assert got.real.tobytes() == want_q.tobytes() and got.imag.tobytes() == want_i.tobytes()
    full = tr.convert(np.array([info.min, info.max], tr.DTYPES[fmt]), fmt)
    assert full.real[0] == -1.0 and 0.99 < full.imag[0] <= 1.0
    assert (tr.SCALES, tr.BYTES) == ((1.0, 1 / 32768, 1 / 128, 1 / 127.5), (8, 4, 2, 2))


def test_the_increment_is_the_rounded_shift():
    assert tr.increment(0.0) == 0 and tr.increment(0.5) == tr.increment(-0.5) == 2 ** 63
    assert tr.increment(0.25) == 2 ** 62 and tr.increment(-0.25) == 3 * 2 ** 62
    assert tr.increment(2.0 ** -40) == 2 ** 24 and tr.increment(-2.0 ** -64) == 2 ** 64 - 1
    assert tr.increment(2.0 ** -65) == 0 and tr.increment(3 * 2.0 ** -65) == 2              # ties to even
    assert tr.increment(0.05) == round(0.05 * 2 ** 64)                                        # (Python's float -> int product is exact here: 0.05 2^64 < 2^63)


def test_a_tone_at_the_captures_offset_lands_at_dc():
    # a 10 Msps int16 capture whose channel centre lies 250 kHz above the capture's: the carrier of the channel at half of full scale
    rate, offset, N = 10e6, 250e3, 40000
    n = np.arange(N, dtype=np.float64)
    tone = 0.5 * np.exp(2j * math.pi * offset / rate * n)
    raw = np.empty(2 * N, np.int16)
    raw[0::2], raw[1::2] = np.rint(tone.real * 32768), np.rint(tone.imag * 32768)
    taps = tr.design(32, 35)
    y = tr.tuner(raw, tr.CS16, 32, 35, shift=-offset / rate, taps=taps)[2 * len(taps) // 35 + 2:]
    mean = y.astype(np.complex128).mean()
    # gain: the pass band's ripple (0.06 dB) and the branches' spread around 1 (the prototype's stop band at the multiples of 1 / L, -69 dB = 0.003 dB)
    assert abs(20.0 * math.log10(abs(mean) / 0.5)) <= 0.07
    # at 0 Hz: what moves is the images at -69 dB (3.5e-4), the quantisation noise (2^-16 / 0.5 rms before the filter) and float32
    assert np.abs(y - mean).max() <= 1e-3 * abs(mean)
    assert abs(np.angle(mean)) < 1e-3
    # ... and without the shift it stays where it was, 250 kHz = 0.02734 cycles per output sample
    y0 = tr.tuner(raw, tr.CS16, 32, 35, taps=taps)[100:]
    step = np.angle((y0[1:].astype(np.complex128) * np.conj(y0[:-1].astype(np.complex128))).mean()) / (2 * math.pi)
    assert abs(step - offset / rate * 35 / 32) < 1e-6


def test_a_tone_in_the_stop_band_is_down_by_the_designed_attenuation():
    # 16/35 (a 20 Msps capture): the stop band begins at 0.58 * 16 / 35 = 0.265 cycles per input sample
    N = 30000
    taps = tr.design(16, 35)
    lead = 2 * len(taps) // 35 + 2
    for f in (0.27, 0.3, -0.41, 0.5):
        tone = np.exp(2j * math.pi * f * np.arange(N, dtype=np.float64)).astype(np.complex64)
        y = tr.tuner(tone, tr.CF32, 16, 35, taps=taps)[lead:]
        assert len(y) > 13000
        assert np.abs(y).max() <= 10.0 ** (-(tr.ATTEN_DB - 1.0) / 20.0), f
    tone = np.exp(2j * math.pi * 0.1 * np.arange(N, dtype=np.float64)).astype(np.complex64)      # 0.219 of the output rate: the pass band
    y = tr.tuner(tone, tr.CF32, 16, 35, taps=taps)[lead:]
    assert abs(20.0 * math.log10(np.abs(y).max())) <= 0.07 and abs(20.0 * math.log10(np.abs(y).min())) <= 0.07


# ------------------------------------------------------------------ through the oracle
def test_a_capture_tuned_by_the_model_decodes_to_the_originals_ts(po):
    c = po.cfg(po.QAM16, po.C1_2, po.T2k)
    src = po.stream_slice(c, 4, 13)
    ref = po.rx(c, src, snr_db=30, want=("ts",))["ts"]
    up = tr.tuner(src, tr.CF32, 35, 32)
    raw = tr.capture_cs16(up, 0.05)
    assert raw.dtype == np.int16 and max(abs(int(raw.max())), abs(int(raw.min()))) == 16384
    iq = tr.tuner(raw, tr.CS16, 32, 35, shift=-0.05)
    assert len(iq) == tr.outputs(len(up), 32, 35) and abs(len(iq) - len(src)) <= 1
    ts = po.rx(c, iq, snr_db=30, want=("ts",))["ts"]
    assert len(ts) > 0
    n = tr.ts_common_packets(ts, ref)
    print(f"\n{len(ts) // 188} packets from the tuned capture, {len(ref) // 188} from the original, {n} in common")
    assert n >= 2 * po.packets_per_superframe(c)
