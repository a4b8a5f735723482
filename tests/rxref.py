"""Plain references for the receive-block tests (a helper module, not a test file).

- an RS(204,188) word corpus: encoded with the oracle's o_rs_encode, then given a chosen number of byte errors per word at chosen places, with a chosen
  number of bad words in every 64-word wavefront (the reed_solomon_dec launch picks its decoder per wavefront: k_backend.hpp, RS_LANE_MIN);
- energy_descramble's general_work (lib/energy_descramble_impl.cc) restated one call at a time, so that a stream delivered in calls of any size can
  be compared byte for byte, with the block's consumed / produced counts;
- the K = 7 convolutional code with the puncturing of the code rate, mapped to d_m-bit symbols (the Viterbi decoder's input).
"""
import ctypes as C

import numpy as np

WAVE = 64                  # RS words per wavefront of the decoder's launch
RS_LANE_MIN = 24           # bad words per wavefront from which every lane decodes its own word (k_backend.hpp)
NSYNC, SYNC = 0xB8, 0x47
GROUP = 8 * 188            # one energy_descramble item: 8 packets


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- RS corpus
def _positions(rng, nerr, where):
    """indices (in the 204-byte shortened word) of nerr distinct bytes: 'random', 'first' (payload byte 0 and others), 'last' (the last parity byte
    and others), 'burst' (nerr adjacent bytes), 'parity' (parity bytes only, 188..203)"""
    if where == "random":
        return rng.choice(204, nerr, replace=False)
    if where == "first":
        return np.concatenate([[0], 1 + rng.choice(203, nerr - 1, replace=False)])
    if where == "last":
        return np.concatenate([[203], rng.choice(203, nerr - 1, replace=False)])
    if where == "burst":
        s = rng.randint(0, 204 - nerr + 1)
        return np.arange(s, s + nerr)
    if where == "parity":
        return 188 + rng.choice(16, nerr, replace=False)
    raise ValueError(where)


def rs_corpus(po, nwords, bad_per_wave, errors=tuple(range(1, 17)), where="random", garbage_every=0, seed=0):
    """nwords RS(204,188) words (the shortened RS(255,239) of DVB-T).  In every 64-word wavefront (the last one may be partial) exactly
    min(bad_per_wave, its size) words are bad: they carry errors[j % len(errors)] byte errors at `where`, and every garbage_every-th bad word is
    replaced by uniform random bytes.  Returns a dict: words [nwords, 204], payload [nwords, 188] (what was transmitted), nerr [nwords] (0 for a
    clean word, -1 for garbage), and bad_per_wave, the bad-word count of every wavefront (asserted to be what was asked for)."""
    assert all(1 <= e <= 16 for e in errors)
    L = po.lib()
    rs = po.RS()
    L.o_rs_init(C.byref(rs))
    rng = np.random.RandomState(seed)
    payload = rng.randint(0, 256, (nwords, 188)).astype(np.uint8)
    words = np.zeros((nwords, 204), np.uint8)
    cw = np.zeros(255, np.uint8)
    par = np.zeros(16, np.uint8)
    for w in range(nwords):
        cw[:] = 0
        cw[51:239] = payload[w]
        L.o_rs_encode(C.byref(rs), _p(cw), _p(par))
        words[w, :188] = payload[w]
        words[w, 188:] = par
    nerr = np.zeros(nwords, np.int32)
    j = 0
    for w0 in range(0, nwords, WAVE):
        size = min(WAVE, nwords - w0)
        for w in w0 + np.sort(rng.choice(size, min(bad_per_wave, size), replace=False)):
            j += 1
            if garbage_every and j % garbage_every == 0:
                words[w] = rng.randint(0, 256, 204)
                nerr[w] = -1
                continue
            e = errors[(j - 1) % len(errors)]
            for q in _positions(rng, e, where):
                words[w, q] ^= rng.randint(1, 256)
            nerr[w] = e
    bad = np.array([(nerr[w0:w0 + WAVE] != 0).sum() for w0 in range(0, nwords, WAVE)])
    want = np.array([min(bad_per_wave, min(WAVE, nwords - w0)) for w0 in range(0, nwords, WAVE)])
    assert (bad == want).all(), (bad, want)
    return {"words": words, "payload": payload, "nerr": nerr, "bad_per_wave": bad}


def rs_path(bad_in_wave):
    """the decoder a wavefront with this many bad words runs (no defer list: the per-block entry)"""
    return "lane" if bad_in_wave >= RS_LANE_MIN else ("wave" if bad_in_wave else "none")


# ---------------------------------------------------------------- energy_descramble, call by call
def prbs_group():
    """the XOR mask of one group of 8 packets: PRBS 1 + x^14 + x^15 from 100101010000000, clocked 8 times per byte (the first bit the most
    significant); the sync bytes are not scrambled (0 in the mask) and the first packet's is not clocked -- ETSI EN 300 744 4.3.1"""
    reg = 0xa9
    mask = np.zeros(GROUP, np.uint8)

    def clock8():
        nonlocal reg
        byte = 0
        for _ in range(8):
            fb = ((reg >> 13) ^ (reg >> 14)) & 1
            reg = ((reg << 1) | fb) & 0x7fff
            byte = (byte << 1) | fb
        return byte
    for p in range(8):
        for k in range(1, 188):
            mask[p * 188 + k] = clock8()
        clock8()                                 # the next packet's sync byte: clocked, not used
    return mask


def descramble_calls(stream, calls, d_index=0):
    """energy_descramble_impl.cc general_work, one call at a time, written from its rule: the input is `stream` (bytes, items of 1504) read from
    the front; calls[i] is the i-th call's noutput_items in items (a multiple of 4: set_output_multiple(4 * 1504)).  A call is made only while the
    input holds at least that many items.  Every call looks for an NSYNC (0xB8) at its offset d_index and on at 188-byte strides within its first
    two items; none found: d_index back to 0, two items consumed, nothing produced.  Found: nout - 2 items consumed and nout - 2 items delivered,
    read from d_index on, the first byte of every packet 0x47 and the rest XORed with the group's PRBS.  d_index is kept for the next call.
    Returns (list of (consumed items, produced bytes, the bytes), the final d_index)."""
    mask = prbs_group()
    x = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else stream
    pos, res = 0, []
    for k in calls:
        assert k % 4 == 0 and k >= 4
        if (len(x) - pos) // GROUP < k:
            break
        w = x[pos:]
        while d_index < 2 * GROUP and w[d_index] != NSYNC:
            d_index += 188
        if d_index >= 2 * GROUP:
            d_index = 0
            res.append((2, 0, np.zeros(0, np.uint8)))
            pos += 2 * GROUP
            continue
        n = k - 2
        src = w[d_index:d_index + n * GROUP].reshape(n, GROUP)
        out = src ^ mask[None, :]
        out[:, ::188] = SYNC
        res.append((n, n * GROUP, out.reshape(-1)))
        pos += n * GROUP
    return res, d_index


# ---------------------------------------------------------------- inner code
def conv_encode(bits):
    """K = 7 mother code, G1 = 171, G2 = 133 (octal), encoder starting from zero: (x, y) per input bit"""
    u = np.concatenate([np.zeros(6, np.uint8), bits.astype(np.uint8)])
    n = len(bits)

    def tap(d):
        return u[6 - d:6 - d + n]
    x = tap(0) ^ tap(1) ^ tap(2) ^ tap(3) ^ tap(6)
    y = tap(0) ^ tap(2) ^ tap(3) ^ tap(5) ^ tap(6)
    return x, y


def coded_symbols(po, c, nbytes, ber, seed, m=None):
    """nbytes random bytes through the mother code and the puncturing of c.code_rate, bits flipped with probability ber, packed into m-bit
    symbols (m = c.m by default; the first bit the most significant).  Returns (the bytes, the symbols)."""
    m = c.m if m is None else m
    rng = np.random.RandomState(seed)
    data = rng.randint(0, 256, nbytes).astype(np.uint8)
    x, y = conv_encode(np.unpackbits(data))
    inter = np.empty(2 * len(x), np.uint8)
    inter[0::2] = x
    inter[1::2] = y
    ln = C.c_int()
    po.lib().o_vit_puncture.restype = C.POINTER(C.c_ubyte)
    pp = po.lib().o_vit_puncture(c.code_rate, C.byref(ln))
    punct = np.array([pp[i] for i in range(ln.value)], np.uint8)
    keep = np.tile(punct, len(inter) // len(punct) + 1)[:len(inter)].astype(bool)
    kept = inter[keep] ^ (rng.rand(keep.sum()) < ber).astype(np.uint8)
    nsym = len(kept) // m
    sym = np.zeros(nsym, np.uint8)
    for j in range(m):
        sym |= kept[j:nsym * m:m] << (m - 1 - j)
    return data, sym


# ---------------------------------------------------------------- rational resampler + multiply_const (k_resample.hpp), float64
RS_MAX_BRANCH_FLOATS = 64 * 48     # k_resample.hpp: floats of the branch table a workgroup stages (ri * nt must fit)
RS_TILE_IN = 768                   # k_resample.hpp: input samples a workgroup of 256 outputs stages


def resampler_design64(interp, decim):
    """rational_resampler(interp, decim, taps=None, fractional_bw=None) of the GNU Radio 3.7 series, as the header comment of resampler_taps
    (dvbt_tables.hpp) names it, in float64 throughout: interp / decim reduced by their gcd; fractional_bw 0.4; design_filter = firdes.low_pass(gain
    ri, fs ri, mid, width, Kaiser beta 7) with width = 0.1 and mid = 0.45 for a rate >= 1, both times the rate below; compute_ntaps =
    int((beta / 0.1102 + 8.7) fs / (22 width)) made odd; low_pass = sin(n w0) / (n pi) under the Kaiser window, w0 = 2 pi mid / fs, normalised to
    the gain at DC.  Returns (taps, ri, rd, nt): the prototype, the reduced ratio and the taps per polyphase branch, ceil(len(taps) / ri)."""
    g = int(np.gcd(interp, decim))
    ri, rd = interp // g, decim // g
    fractional_bw, beta, halfband = 0.4, 7.0, 0.5
    rate = ri / rd
    if rate >= 1.0:
        width = halfband - fractional_bw
        mid = halfband - width / 2.0
    else:
        width = rate * (halfband - fractional_bw)
        mid = rate * halfband - width / 2.0
    fs = float(ri)
    ntaps = int((beta / 0.1102 + 8.7) * fs / (22.0 * width))
    ntaps += 1 - (ntaps & 1)
    n = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) // 2
    taps = 2.0 * mid / fs * np.sinc(2.0 * mid / fs * n) * np.kaiser(ntaps, beta)
    taps *= ri / taps.sum()
    return taps, ri, rd, (ntaps + ri - 1) // ri


def resampler_supported(ri, rd, nt):
    """the support rule of ResamplerDesign::build (dvbt_hip.hip): the branch table and the input tile of one workgroup fit their LDS arrays"""
    return ri * nt <= RS_MAX_BRANCH_FLOATS and 256 * rd // ri + nt + 2 <= RS_TILE_IN


def resample64(x, taps, ri, rd, scale):
    """out[M] = scale * sum_k branch[(M rd) mod ri][k] * x[floor(M rd / ri) - k], branch[b][k] = taps[b + k ri] (0 past the end), x = 0 outside
    [0, len), M = 0 .. ceil(len ri / rd) - 1, in complex128.  Returns (out, A_re, A_im): A_re[M] = |scale| sum_k |branch[..][k]| |Re x[..]|, the
    sum of the magnitudes of what out[M].real adds up (the scale of its rounding error), A_im likewise.
    Every branch at every input position as one matrix product over the windows x[n - nt + 1 .. n], of which each output picks its own."""
    x = np.asarray(x).astype(np.complex128)
    taps = np.asarray(taps, np.float64)
    nt = (len(taps) + ri - 1) // ri
    br = np.zeros(ri * nt)
    br[:len(taps)] = taps
    br = br.reshape(nt, ri).T                                  # br[b][k] = taps[b + k ri]
    nout = (len(x) * ri + rd - 1) // rd
    M = np.arange(nout, dtype=np.int64)
    n_of, b_of = M * rd // ri, M * rd % ri                     # n_of < len(x)
    flipped = np.ascontiguousarray(br[:, ::-1].T)              # window column j holds x[n - (nt - 1 - j)]

    def every_branch(v, t):
        w = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(np.concatenate([np.zeros(nt - 1), v]), nt))
        return (w @ t)[n_of, b_of]
    out = every_branch(x.real, flipped) + 1j * every_branch(x.imag, flipped)
    a_re, a_im = every_branch(np.abs(x.real), np.abs(flipped)), every_branch(np.abs(x.imag), np.abs(flipped))
    return out * scale, a_re * abs(scale), a_im * abs(scale)


def resample_bound(a, nt):
    """how far a float32 evaluation of resample64 may lie from it, per output and component: nt products and nt - 1 additions in any order, fused or
    not, each rounding by at most 2^-24 of a partial sum that the magnitude sum a bounds (first order: nt 2^-24 a), one more rounding for the scale,
    one of margin for the higher-order terms; 2^-149 for a result flushed to zero"""
    return (nt + 2) * 2.0 ** -24 * a + 2.0 ** -149


def resampler_call_count(ri, rd, produced, consumed, nout, nin):
    """what a work() call must produce, from the block's contract alone: output M can be produced once input floor(M rd / ri) has been offered.
    `produced` outputs exist and `consumed` inputs were taken by earlier calls, so this call offers the inputs below consumed + nin; the outputs
    M >= produced whose newest input floor(M rd / ri) lies below that are those with M rd < (consumed + nin) ri"""
    if nout <= 0 or nin <= 0:
        return 0
    offered = consumed + nin
    ready = (offered * ri - 1) // rd + 1 - produced            # M = produced .. (offered ri - 1) // rd
    return max(0, min(nout, ready))
