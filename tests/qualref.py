"""Model of the blind signal-quality figures (numpy only): the specification of dvbt_rx_quality.

All three figures are functions of taps the receive chain already has:
  MER            equalised carriers (EQ) against the nearest constellation point,
  channel errors the Viterbi decoder's output (VITERBI) re-encoded against its input (BITDEINT),
  post errors    the byte de-interleaver's output (DEINT, or regathered from VITERBI) against the RS decoder's output (RS).
"""
import numpy as np

# puncture vectors of the five code rates (X, Y interleaved per step, period 2k) and k of rate k / (k + 1)
PUNCT = {0: (1, 1), 1: (1, 1, 0, 1), 2: (1, 1, 0, 1, 1, 0), 3: (1, 1, 0, 1, 1, 0, 0, 1, 1, 0),
         4: (1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0)}
RATE_K = {0: 1, 1: 2, 2: 3, 3: 5, 4: 7}
X_DELAYS = (0, 1, 2, 3, 6)          # 171 octal
Y_DELAYS = (0, 2, 3, 5, 6)          # 133 octal
NORM = {2: 1.0 / np.sqrt(2.0), 4: 1.0 / np.sqrt(10.0), 6: 1.0 / np.sqrt(42.0)}     # non-hierarchical modes


def mer(eq, m, norm=None):
    """(mer_carriers, mer_signal, mer_error) of equalised carriers (complex, any shape) of a 2^m-point constellation:
    ideal = the nearest point of the grid (2 i + 1 - L) norm per axis, L = 2, 4, 8."""
    eq = np.asarray(eq).reshape(-1)
    L = 1 << (m // 2)
    nrm = float(np.float32(NORM[m] if norm is None else norm))

    def nearest(x):
        i = np.clip(np.floor(x / (2.0 * nrm) + L / 2.0), 0, L - 1)
        return (2.0 * i + 1.0 - L) * nrm
    re, im = eq.real.astype(np.float64), eq.imag.astype(np.float64)
    ire, iim = nearest(re), nearest(im)
    sig = float(np.sum(ire * ire + iim * iim))
    err = float(np.sum((re - ire) ** 2 + (im - iim) ** 2))
    return int(eq.size), sig, err


def mer_db(sig, err):
    return float("inf") if err <= 0 else 10.0 * float(np.log10(sig / err))


def info_bits(vit):
    """decoded bytes -> information bits, MSB first: bit t of the stream is trellis step t"""
    return np.unpackbits(np.asarray(vit, np.uint8))


def encode(bits):
    """(X, Y) of every step of the K = 7 mother code; steps with fewer than six predecessors see zeros in front"""
    u = np.concatenate([np.zeros(6, np.uint8), np.asarray(bits, np.uint8)])
    n = len(bits)
    x = np.zeros(n, np.uint8)
    y = np.zeros(n, np.uint8)
    for d in X_DELAYS:
        x ^= u[6 - d:6 - d + n]
    for d in Y_DELAYS:
        y ^= u[6 - d:6 - d + n]
    return x, y


def kept_positions(n_steps, code_rate):
    """coded positions c = 2 t (X), 2 t + 1 (Y) of steps [0, n_steps) that the puncture vector keeps, in stream order:
    the q-th entry is where kept bit q comes from"""
    p = np.array(PUNCT[code_rate], np.uint8)
    c = np.arange(2 * n_steps)
    return c[p[c % len(p)] == 1]


def puncture_pack(bits, code_rate, m):
    """encode, puncture and pack into bytes of m bits (MSB first), as the decoder receives them; a last partial byte is dropped"""
    x, y = encode(bits)
    coded = np.empty(2 * len(bits), np.uint8)
    coded[0::2] = x
    coded[1::2] = y
    kept = coded[kept_positions(len(bits), code_rate)]
    nb = len(kept) // m
    w = (1 << np.arange(m - 1, -1, -1)).astype(np.uint8)
    return (kept[:nb * m].reshape(nb, m) * w).sum(axis=1).astype(np.uint8)


def unpack_input(inp, m):
    """decoder input bytes -> the kept-bit stream: byte q // m, bit m - 1 - q % m"""
    inp = np.asarray(inp, np.uint8).reshape(-1)
    sh = np.arange(m - 1, -1, -1)
    return ((inp[:, None] >> sh[None, :]) & 1).astype(np.uint8).reshape(-1)


FIRST_STEP = 8      # the first counted step: the first whole decoded byte behind the six bits the encoder needs (step 6 is the first with six predecessors)


def counted_set(n_vit, n_in, m, code_rate, first_step=FIRST_STEP):
    """(kept-bit indices q, coded positions c) of the counted set: steps first_step <= t < 8 n_vit whose kept bit lies inside the input"""
    if n_vit < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = kept_positions(8 * n_vit, code_rate)
    q = np.arange(len(c))
    sel = (c >= 2 * first_step) & (q < n_in * m)
    return q[sel], c[sel]


def channel_errors(inp, vit, m, code_rate, first_step=FIRST_STEP):
    """(channel_bits, channel_bit_errors): the decoder's output `vit` re-encoded against its input `inp`"""
    inp = np.asarray(inp, np.uint8).reshape(-1)
    vit = np.asarray(vit, np.uint8).reshape(-1)
    q, c = counted_set(len(vit), len(inp), m, code_rate, first_step)
    if len(q) == 0:
        return 0, 0
    x, y = encode(info_bits(vit))
    coded = np.empty(2 * len(x), np.uint8)
    coded[0::2] = x
    coded[1::2] = y
    rx = unpack_input(inp[:(int(q[-1]) // m) + 1], m)
    return int(len(q)), int(np.count_nonzero(coded[c] != rx[q]))


def deint_from_viterbi(vit, n_words):
    """the byte de-interleaver in closed form: deint[p] = vit[p - 204 (11 - p % 12)], 0 where that index is negative"""
    vit = np.asarray(vit, np.uint8).reshape(-1)
    p = np.arange(204 * n_words)
    src = p - 204 * (11 - p % 12)
    ok = (src >= 0) & (src < len(vit))
    out = np.zeros(len(p), np.uint8)
    out[ok] = vit[src[ok]]
    return out


_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def post_errors(deint, rs):
    """(post_bits, post_bit_errors): the 188 data bytes of every RS word before and behind the RS decoder"""
    rs = np.asarray(rs, np.uint8).reshape(-1, 188)
    w = len(rs)
    d = np.asarray(deint, np.uint8).reshape(-1)[:204 * w].reshape(w, 204)[:, :188]
    return 1504 * w, int(_POP[d ^ rs].sum())
