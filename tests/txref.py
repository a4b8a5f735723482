"""Plain references for the transmit-side tests (a helper module, not a test file).

- the shifted FFT / IFFT of dvbt_fft in complex128 (numpy) and in complex64 (torch on the CPU), and the relative RMS error that compares them;
- the OFDM baseband of the modulator from its frequency-domain frames: IFFT, cyclic prefix, scale, in float64 and in float32;
- the TPS word of a frame read back from its carriers (DBPSK) and the BCH(67,53) remainder of ETSI EN 300 744 4.6.3.

The float32 figures calibrate the GPU's accuracy bounds: a kernel is held to K times the error of an ordinary float32 FFT of the same input.
"""
import ctypes as C

import numpy as np


def fft64(x, forward):
    """dvbt_fft(shift = 1) in complex128 over the last axis: forward out[b] = X[(b - N/2) mod N]; inverse out[t] = sum_k x[(k + N/2) mod N] e^{+2 pi i t k / N}"""
    x = np.asarray(x).astype(np.complex128)
    N = x.shape[-1]
    if forward:
        return np.fft.fftshift(np.fft.fft(x, axis=-1), axes=-1)
    return np.fft.ifft(np.fft.ifftshift(x, axes=-1), axis=-1) * N


def fft32(x, forward):
    """the same transform as an ordinary float32 FFT computes it (torch.fft on the CPU, complex64)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex64))
    N = t.shape[-1]
    if forward:
        return torch.fft.fftshift(torch.fft.fft(t, dim=-1), dim=-1).numpy()
    return (torch.fft.ifft(torch.fft.ifftshift(t, dim=-1), dim=-1) * N).numpy()


def rel_rms(a, ref):
    """||a - ref||_2 / ||ref||_2 in float64"""
    a = np.asarray(a).astype(np.complex128).reshape(-1)
    ref = np.asarray(ref).astype(np.complex128).reshape(-1)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def tone(N, k, sign):
    """e^{sign 2 pi i k n / N}, n = 0 .. N-1, with the phase reduced mod N in integers first"""
    n = np.arange(N, dtype=np.int64)
    return np.exp(sign * 2j * np.pi * ((k * n) % N) / N)


def single_bin_output(N, b, forward):
    """what dvbt_fft(shift = 1) makes of a unit impulse at input index b: forward, out[j] = X[(j - N/2) mod N] = e^{-2 pi i b (j - N/2) / N};
    inverse, input b is IFFT bin (b - N/2) mod N, out[t] = e^{+2 pi i t (b - N/2) / N}"""
    if forward:
        return tone(N, b, -1) * (-1.0) ** b
    return tone(N, (b - N // 2) % N, +1)


def _with_cp(t, cp):
    return np.concatenate([t[:, t.shape[1] - cp:], t], axis=1).reshape(-1)


def baseband64(carriers, cp, scale):
    """the modulator's output for frequency-domain frames carriers[nsym, N] (carrier c at column zeros_on_left + c): ifft(ifftshift) unnormalised,
    the last cp samples in front, times scale -- complex128"""
    return _with_cp(fft64(carriers, forward=False), cp) * float(scale)


def baseband32(carriers, cp, scale):
    """baseband64 as a float32 pipeline computes it: complex64 IFFT (torch CPU), then scale in float32"""
    return (_with_cp(fft32(carriers, forward=False), cp) * np.float32(scale)).astype(np.complex64)


# ---------------------------------------------------------------- TPS
BCH_G = 0b100001101110111             # x^14 + x^9 + x^8 + x^6 + x^5 + x^4 + x^2 + x + 1 (ETSI EN 300 744 4.6.3)


def bch_remainder(bits):
    """remainder of s1 .. s67 (s1 = highest power) divided by the BCH generator: 0 for a codeword"""
    r = 0
    for b in bits:
        r = (r << 1) | int(b)
        if r & (1 << 14):
            r ^= BCH_G
    return r


def tps_carriers(po, c):
    """the TPS carriers of the configuration and the reference sequence w_k at them"""
    L = po.lib()
    wk = np.zeros(c.Kmax + 1, np.int8)
    L.o_prbs_wk(C.byref(c), wk.ctypes.data_as(C.c_void_p))
    car = np.array([c.tps[i] for i in range(c.n_tps)])
    return car, wk[car]


def decode_tps(frame, zl, car, wk):
    """the TPS bits s1 .. s67 of one frame (at indices 1 .. 67) from its 68 frequency-domain symbols (frame[s, zl + k]): s_j = 1 where the carriers'
    sign flips from symbol j - 1 to j (DBPSK, 4.6).  Index 0 is not a transmitted bit: it is 0 when the first symbol holds the DBPSK initialisation
    2 (1/2 - w_k) of 4.6.  Every TPS carrier must carry the same word."""
    v = frame[:, zl + car].astype(np.complex128)
    assert np.allclose(v.imag, 0.0) and np.allclose(np.abs(v.real), 1.0), "TPS carriers are real, +-1"
    sgn = np.sign(v.real).astype(np.int64)                        # [68, n_tps]
    s0 = (sgn[0] != (1 - 2 * wk.astype(np.int64))).astype(np.uint8)
    flips = (sgn[1:] != sgn[:-1]).astype(np.uint8)
    assert (flips == flips[:, :1]).all() and (s0 == s0[0]).all(), "the TPS carriers disagree"
    return np.concatenate([[s0[0]], flips[:, 0]]).astype(np.uint8)


def tps_field(t, first, last):
    """s_first .. s_last as an integer, s_first the MSB"""
    v = 0
    for b in t[first:last + 1]:
        v = (v << 1) | int(b)
    return v
