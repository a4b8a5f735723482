"""The channel block's specification as a numpy model (include/dvbt_hip.h, dvbt_channel_*): integer Philox4x32-10, the phase as a Python-int product,
everything else in float64.

    e[n] = x[n] + sum_i a_i x[n - d_i]                 x[k] = 0 in front of the stream's first sample
    r[n] = e[n] exp(2 pi j phi(n))                     phi(n) = (inc n mod 2^64) / 2^64, inc = round(cfo / fft_length 2^64) mod 2^64
    y[n] = r[n] + sigma (g_re(n) + j g_im(n))

n is the absolute sample index: first_sample + the index in the array.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or ints) of 32-bit words, key: two 32-bit ints -> uint32 array [..., 4]"""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(rounds):
        p0 = c[0] * np.uint64(M0)                      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return np.stack(c, axis=-1).astype(np.uint32)


def noise(seed, first_sample, count):
    """g_re(n) + j g_im(n) for n = first_sample .. first_sample + count - 1, complex128, unit variance per component"""
    seed = int(seed) & 0xffffffffffffffff
    n = int(first_sample) + np.arange(count, dtype=np.uint64) if count else np.zeros(0, np.uint64)
    if count and int(first_sample) + count > 2 ** 63:
        raise ValueError("sample index beyond 2^63")
    blk = n >> np.uint64(1)
    w = philox4x32((blk & MASK, blk >> np.uint64(32), 0, 0), (seed & 0xffffffff, seed >> 32)).reshape(-1, 4)
    odd = (n & np.uint64(1)).astype(bool)
    wa = np.where(odd, w[:, 2], w[:, 0]).astype(np.uint32)
    wb = np.where(odd, w[:, 3], w[:, 1]).astype(np.uint32)
    u1 = ((wa >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (wb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    return rho * np.cos(2.0 * np.pi * u2) + 1j * rho * np.sin(2.0 * np.pi * u2)


def phase_inc(cfo, fft_length):
    return int(round(cfo / fft_length * 2.0 ** 64)) % 2 ** 64 if cfo else 0


def phasor(cfo, fft_length, first_sample, count):
    """exp(2 pi j phi(n)), complex128: the 64-bit phase is exact, its conversion to an angle keeps 53 bits"""
    inc = phase_inc(cfo, fft_length)
    top = np.array([((inc * (int(first_sample) + i)) % 2 ** 64) >> 11 for i in range(count)], dtype=np.float64) * 2.0 ** -53
    return np.exp(2j * np.pi * top)


def channel(x, echoes=(), cfo=0.0, fft_length=0, noise_sigma=0.0, seed=0, first_sample=0):
    """the model: complex128 out (the block rounds to complex64)"""
    x = np.asarray(x).astype(np.complex128)
    e = x.copy()
    for d, a in echoes:
        if d < len(x):
            e[d:] += complex(a) * x[:len(x) - d]
    if cfo:
        e = e * phasor(cfo, fft_length, first_sample, len(x))
    if noise_sigma:
        e = e + float(noise_sigma) * noise(seed, first_sample, len(x))
    return e
