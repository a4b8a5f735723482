"""Plain references for the receive-block tests (a helper module, not a test file).

- an RS(204,188) word corpus: encoded with the oracle's o_rs_encode, then given a chosen number of byte errors per word at chosen places, with a chosen
  number of bad words in every 64-word wavefront (the reed_solomon_dec launch picks its decoder per wavefront: k_backend.hpp, RS_LANE_MIN);
- energy_descramble's general_work (lib/energy_descramble_impl.cc) restated one call at a time, so that a stream delivered in calls of any size can
  be compared byte for byte, with the block's consumed / produced counts;
- the K = 7 convolutional code with the puncturing of the code rate, mapped to d_m-bit symbols (the Viterbi decoder's input);
- the float64 form of the rational resampler;
- the outer stage of the segment chain (byte de-interleaver, RS decoder, sync bitmap, descrambler) on a Viterbi byte stream built here: the corpus
  builder, the oracle's primitives in sequence, the descrambler's runs, and a piece's TS from the documented contract of a cut stream.
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


def descramble_calls(stream, calls, d_index=0, trace=None):
    """energy_descramble_impl.cc general_work, one call at a time, written from its rule: the input is `stream` (bytes, items of 1504) read from
    the front; calls[i] is the i-th call's noutput_items in items (a multiple of 4: set_output_multiple(4 * 1504)).  A call is made only while the
    input holds at least that many items.  Every call looks for an NSYNC (0xB8) at its offset d_index and on at 188-byte strides within its first
    two items; none found: d_index back to 0, two items consumed, nothing produced.  Found: nout - 2 items consumed and nout - 2 items delivered,
    read from d_index on, the first byte of every packet 0x47 and the rest XORed with the group's PRBS.  d_index is kept for the next call.
    Returns (list of (consumed items, produced bytes, the bytes), the final d_index).  trace: a list that receives, per call, (the call's first
    item, d_index as the call found it, d_index as it left it or -1 when nothing was found)."""
    mask = prbs_group()
    x = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else stream
    pos, res = 0, []
    for k in calls:
        assert k % 4 == 0 and k >= 4
        if (len(x) - pos) // GROUP < k:
            break
        w = x[pos:]
        d_before = d_index
        while d_index < 2 * GROUP and w[d_index] != NSYNC:
            d_index += 188
        if trace is not None:
            trace.append((pos // GROUP, d_before, d_index if d_index < 2 * GROUP else -1))
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


# ---------------------------------------------------------------- the segment chain's outer stage on a built Viterbi stream
# The stream is what the transmitter's byte interleaver emits in steady state: 11 clean lead-in words, then the corpus, through o_conv_interleave,
# without the first 11 * 204 bytes.  The receiver's de-interleaver (zero-filled branches, as at every stream start) then gives
#   output word w = corpus word w - 11, exactly, for w >= 11;
#   output words 0 .. 10 (the junction words) = lead-in bytes where the branch has filled, zeros elsewhere -- byte 0 always zero, never a codeword
# (asserted by tests/test_outer_corpus.py).  The kernels count their 64-word wavefronts in OUTPUT words, so wavefront 0 holds the 11 junction
# words and corpus words 0 .. 52.
JUNCTION = 11
DESCR_MAX_RUNS = 1024      # k_backend.hpp: the run list's length before it was sized by the stream
WHERES = ("random", "first", "last", "burst", "parity")


def _outer_lib(po):
    L = po.lib()
    L.o_conv_interleave.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_conv_deinterleave.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_rs_dec_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.o_energy_descramble_groups.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_energy_descramble_groups.restype = C.c_size_t
    return L


def rs_encode_words(po, payload):
    """[n, 188] payloads -> [n, 204] RS(204,188) words (o_rs_encode on the zero-padded RS(255,239) word)"""
    L = po.lib()
    rs = po.RS()
    L.o_rs_init(C.byref(rs))
    words = np.zeros((len(payload), 204), np.uint8)
    words[:, :188] = payload
    cw = np.zeros(255, np.uint8)
    par = np.zeros(16, np.uint8)
    for w in range(len(payload)):
        cw[51:239] = payload[w]
        L.o_rs_encode(C.byref(rs), _p(cw), _p(par))
        words[w, 188:] = par
    return words


def dispersed_words(po, n, out_phase, seed):
    """n encoded corpus words as energy dispersal leaves them: byte 0 = 0xB8 in every 8th packet, 0x47 in the others, the rest uniform (a
    scrambled payload is).  out_phase: the NSYNC packets are the OUTPUT words w = corpus index + 11 with w % 8 == out_phase % 8."""
    assert n % 8 == 0
    rng = np.random.RandomState(seed)
    payload = rng.randint(0, 256, (n, 188)).astype(np.uint8)
    payload[:, 0] = SYNC
    payload[(out_phase - JUNCTION) % 8::8, 0] = NSYNC
    return rs_encode_words(po, payload)


def hit_words(words, idx, seed, errors=tuple(range(1, 17)), wheres=WHERES, garbage_every=0, nerr=None):
    """byte errors into words[idx] in place, as rs_corpus applies them: the j-th word gets errors[j % len] errors at wheres[j % len]; every
    garbage_every-th is replaced by uniform bytes.  Returns nerr (0 clean, -1 garbage), updated when given."""
    rng = np.random.RandomState(seed)
    nerr = np.zeros(len(words), np.int32) if nerr is None else nerr
    for j, w in enumerate(idx):
        assert nerr[w] == 0
        if garbage_every and (j + 1) % garbage_every == 0:
            words[w] = rng.randint(0, 256, 204)
            nerr[w] = -1
            continue
        e = errors[j % len(errors)]
        for q in _positions(rng, e, wheres[j % len(wheres)]):
            words[w, q] ^= rng.randint(1, 256)
        nerr[w] = e
    return nerr


def wave_slots(n_out, wave):
    """the corpus indices whose output words lie in wavefront `wave` of a stream of n_out output words"""
    lo, hi = max(wave * WAVE, JUNCTION), min((wave + 1) * WAVE, n_out)
    return np.arange(lo, hi) - JUNCTION


def load_waves(words, n_out, bad_of_wave, seed, **kw):
    """bad_of_wave(wave) corpus words of every output wavefront made bad (as many as the wavefront has, at the most) at random places.  Returns nerr."""
    rng = np.random.RandomState(seed ^ 0x5a5a)
    idx = []
    for wave in range((n_out + WAVE - 1) // WAVE):
        slots = wave_slots(n_out, wave)
        idx.extend(np.sort(rng.choice(slots, min(bad_of_wave(wave), len(slots)), replace=False)))
    return hit_words(words, idx, seed, **kw)


def viterbi_stream(po, corpus, seed=1):
    """the Viterbi byte stream of `corpus` ([n, 204]; n output words).  See the section's header."""
    L = _outer_lib(po)
    lead = rs_encode_words(po, np.random.RandomState(seed + 77).randint(0, 256, (JUNCTION, 188)).astype(np.uint8))
    x = np.ascontiguousarray(np.concatenate([lead, corpus]).reshape(-1))
    y = np.zeros_like(x)
    L.o_conv_interleave(_p(x), _p(y), len(x))
    return np.ascontiguousarray(y[JUNCTION * 204:])


def bad_per_wave(nerr, n_out):
    """bad words of every output wavefront: the junction words and the corpus words with errors"""
    bad = np.ones(n_out, bool)
    bad[JUNCTION:] = nerr[:n_out - JUNCTION] != 0
    return np.array([bad[w:w + WAVE].sum() for w in range(0, n_out, WAVE)])


def deferred_words(bad_waves):
    """words the fused kernel hands to rs_fix_kernel: the bad words of the wavefronts with 1 .. RS_LANE_MIN - 1 of them"""
    return int(sum(b for b in bad_waves if 0 < b < RS_LANE_MIN))


def segment_words(n_bytes):
    """RS words of a segment whose Viterbi stream has n_bytes: an even number of 8-word items (convolutional_deinterleaver, set_output_multiple(2))"""
    return ((n_bytes // 204 // 8) & ~1) * 8


def sync_bitmap(rs, n_words):
    """bit w of the 64-bit words: rs[w, 0] == 0xB8 for w < n_words, 0 above that inside the last word"""
    bits = np.zeros((n_words + 63) // 64 * 64, np.uint8)
    bits[:n_words] = rs[:n_words, 0] == NSYNC
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8")


def rs_decode_words(po, words, compat):
    """o_rs_dec_block over [n, 204] words: (the [n, 188] payloads as the decoder leaves them, words it gave up on, symbols it corrected)"""
    L = _outer_lib(po)
    rs = po.RS()
    L.o_rs_init(C.byref(rs))
    words = np.ascontiguousarray(words)
    out = np.zeros((len(words), 188), np.uint8)
    nf, nc = C.c_int(), C.c_int()
    L.o_rs_dec_block(C.byref(rs), _p(words), _p(out), len(words), compat, C.byref(nf), C.byref(nc))
    return out, nf.value, nc.value


def outer_reference(po, stream, compat, n_words=None, descramble=True):
    """the oracle's primitives in sequence over the first n_words (default: a segment's count) output words of `stream`: o_conv_deinterleave,
    o_rs_dec_block, o_energy_descramble.  Returns a dict: n_words, deint [n, 204], rs [n, 188], fail, corr, bitmap, ts (bytes)."""
    L = _outer_lib(po)
    n = segment_words(len(stream)) if n_words is None else n_words
    de = np.zeros(len(stream), np.uint8)
    L.o_conv_deinterleave(_p(stream), _p(de), len(stream))
    de = np.ascontiguousarray(de[:n * 204]).reshape(n, 204)
    out, nf, nc = rs_decode_words(po, de, compat)
    ref = {"n_words": n, "deint": de, "rs": out, "fail": nf, "corr": nc, "bitmap": sync_bitmap(out, n)}
    if descramble:
        ts = np.zeros(n * 188 + 8, np.uint8)
        m = L.o_energy_descramble(_p(out), n // 8, _p(ts))
        ref["ts"] = ts[:m]
    return ref


def descramble_runs(rs):
    """the descrambler over rs ([n, 188], n a multiple of 8) in the smallest calls it accepts (descramble_calls, 4 items each): the runs of calls
    that deliver from one offset without a gap, as (first packet, packets), the packets whose first byte some call examined, and the delivered bytes"""
    nitems = len(rs) // 8
    trace = []
    res, _ = descramble_calls(rs.reshape(-1), [4] * max(0, (nitems - 2) // 2), trace=trace)
    runs, looked = [], []
    for (_, produced, _), (item, d0, d1) in zip(res, trace):
        first = item * 8
        looked.extend(range(first + d0 // 188, first + (d1 // 188 if d1 >= 0 else 15) + 1))
        if not produced:
            continue
        src = first + d1 // 188
        if runs and runs[-1][0] + runs[-1][1] == src:
            runs[-1][1] += 16
        else:
            runs.append([src, 16])
    ts = np.concatenate([r[2] for r in res]) if res else np.zeros(0, np.uint8)
    return [tuple(r) for r in runs], np.array(sorted(set(looked)), np.int64), ts


def cut_reference(po, rs, phase16):
    """the TS of a piece that continues a cut stream, from the contract (include/dvbt_hip.h: dvbt_rx_cut; gr_dvbt_amd/multi.py: stitch_ts), over
    its n = len(rs) RS words: delivery starts at the first word whose byte 0 is 0xB8 and takes every whole 8-packet group from there; unclean = 1
    iff some call position c == phase16 (mod 16) with c >= 11 and c + 32 <= n has no NSYNC (phase16 < 0: not known, 0).
    Returns (ts_first_packet, the TS bytes, unclean)."""
    L = _outer_lib(po)
    n = len(rs)
    sync = rs[:, 0] == NSYNC if n else np.zeros(0, bool)
    unclean = 0
    if phase16 >= 0:
        unclean = int(any(not sync[c] for c in range(phase16 % 16, n, 16) if c >= JUNCTION and c + 32 <= n))
    hits = np.flatnonzero(sync)
    if len(hits) == 0:
        return 0, np.zeros(0, np.uint8), unclean
    q = int(hits[0])
    groups = (n - q) // 8
    ts = np.zeros(groups * GROUP, np.uint8)
    if groups:
        src = np.ascontiguousarray(rs[q:q + groups * 8]).reshape(-1)
        assert L.o_energy_descramble_groups(_p(src), groups, _p(ts)) == len(ts)
    return q, ts, unclean


# ---- the named corpora of tests/test_outer_corpus.py (which asserts that each is what it claims) and tests/test_gpu_outer.py
LOADS = (1, 12, 13, 23, 24, 25, 64)        # bad corpus words per output wavefront; wavefront 0 has its 11 junction words on top
CLEAN_SIZES = (16, 32, 48, 64, 80, 1040)
LOAD_WORDS = 24 * WAVE + 16
CYCLE = (23, 24, 0, 64)                    # bad words per wavefront, junction words included
RUNS_WORDS, RUNS_TILE, RUNS_KILL = 59904, 112, (32, 88)
LONG_WORDS, LONG_BREAK_CALL = 16 * 8208, 8195
_cases = {}


def _cycle_load(wave):
    return CYCLE[wave % 4] - (JUNCTION if wave == 0 else 0)


def _lost_nsync(po, corpus, out_words, seed):
    """the corpus words behind these output words again as clean words that carry 0x47 where the NSYNC was"""
    rng = np.random.RandomState(seed)
    pay = rng.randint(0, 256, (len(out_words), 188)).astype(np.uint8)
    pay[:, 0] = SYNC
    corpus[np.asarray(out_words, np.int64) - JUNCTION] = rs_encode_words(po, pay)


def _few_errors(rng, word, n, must=()):
    """n byte errors into one word: at the positions `must` (pairs of position and XOR value) and at random others behind byte 0"""
    for q, v in must:
        word[q] ^= v
    for q in 1 + rng.choice(203, n - len(must), replace=False):
        word[q] ^= rng.randint(1, 256)


def _kinds_corpus(po):
    """16 wavefronts, NSYNC at the output words = 0 (mod 8); the descrambler locks at word 16 and calls at every 16th packet.  Wavefronts 1-3: the
    four packets of the call grid lose their NSYNC to a correctable error (restored by the decoder; 4 bad words: the defer list).  4-6: the same
    among 24 words with parity errors (the lane decoder).  7, 8: the call grid's first packet is garbage (the run breaks, the search goes on) and
    the 7 packets behind it arrive with 0xB8 at byte 0 and at most 8 errors (removed by the decoder; 8 bad words); 9, 10: the same among 20 more."""
    n_out = 16 * WAVE
    corpus = dispersed_words(po, n_out, 0, 31)
    nerr = np.zeros(n_out, np.int32)
    rng = np.random.RandomState(32)
    d = 0                                                         # the descrambler's offset in packets: every break moves it by 8

    def hit(w, n, must=()):
        _few_errors(rng, corpus[w - JUNCTION], n, must)
        nerr[w - JUNCTION] = n

    def fill(wave, count, taken):
        free = np.setdiff1d(np.arange(wave * WAVE, (wave + 1) * WAVE), taken)
        for w in rng.choice(free, count, replace=False):
            for q in 188 + rng.choice(16, 1 + rng.randint(8), replace=False):
                corpus[w - JUNCTION, q] ^= rng.randint(1, 256)
            nerr[w - JUNCTION] = 1
    for wave in range(1, 11):
        if wave <= 6:
            grid = [wave * WAVE + d + 16 * i for i in range(4)]
            for i, w in enumerate(grid):
                hit(w, 1 + (3 * i + wave) % 8, must=((0, 1 + rng.randint(255)),))
            if wave >= 4:
                fill(wave, 24, grid)
        else:
            g = wave * WAVE + d
            corpus[g - JUNCTION] = rng.randint(0, 256, 204)
            corpus[g - JUNCTION, 0] = 0
            nerr[g - JUNCTION] = -1
            for i in range(1, 8):
                hit(g + i, 1 + (i + wave) % 8, must=((0, 0xff),))
            if wave >= 9:
                fill(wave, 20, np.arange(g, g + 8))
            d ^= 8
    return corpus, nerr


def outer_case(po, name):
    """a named corpus: dict with stream (the Viterbi bytes), n_out (output words of the stream), corpus (the words as received), nerr per corpus
    word (0 clean, -1 garbage) and, for the cases made by load_waves, sent (the words before the errors).  Built once per name."""
    if name in _cases:
        return _cases[name]
    kind, _, arg = name.partition("-")
    seed = sum(name.encode()) + 1000
    sent = None
    if kind == "clean":
        n_out = int(arg)
        corpus, nerr = dispersed_words(po, n_out, 0, seed), np.zeros(n_out, np.int32)
    elif kind == "load":                                         # 24 whole wavefronts and one of 16 words, `arg` bad corpus words in each
        n_out = LOAD_WORDS
        corpus = dispersed_words(po, n_out, 0, seed)
        sent = corpus.copy()
        nerr = load_waves(corpus, n_out, lambda wave: int(arg), seed, garbage_every=9)
    elif kind in ("cycle", "range"):                             # wavefronts of 23 / 24 / 0 / 64 bad words in turn: both decoders in one launch
        n_out = LOAD_WORDS if kind == "cycle" else 2000
        corpus = dispersed_words(po, n_out, 0, seed)
        sent = corpus.copy()
        nerr = load_waves(corpus, n_out, _cycle_load, seed, garbage_every=9)
    elif kind == "phase":                                        # clean, the NSYNC packets at the output words = arg (mod 8)
        n_out = 320
        corpus, nerr = dispersed_words(po, n_out, int(arg), seed), np.zeros(n_out, np.int32)
    elif kind == "kinds":
        corpus, nerr = _kinds_corpus(po)
        n_out = len(corpus)
    elif kind in ("nosync", "jump", "both"):                     # 48 packets in a row without NSYNC / `arg` words missing in mid-stream / both
        n_out = 640
        corpus = dispersed_words(po, n_out, 0, seed)
        if kind != "jump":
            _lost_nsync(po, corpus, range(160, 208, 8), seed)
        if kind != "nosync":
            k = int(arg) if arg else 5
            corpus = np.concatenate([corpus[:389], corpus[389 + k:]])
            n_out -= k
        nerr = np.zeros(n_out, np.int32)
    elif kind == "runs":                                         # a tile of 112 words with two lost NSYNC, each on the call grid as the break before leaves it
        tile = dispersed_words(po, RUNS_TILE, 0, seed)           # (tile word i is the output words 11 + i + 112 k)
        _lost_nsync(po, tile, RUNS_KILL, seed)
        n_out = RUNS_WORDS
        corpus, nerr = np.tile(tile, (n_out // RUNS_TILE + 1, 1))[:n_out], np.zeros(n_out, np.int32)
    elif kind == "long":                                         # one run of LONG_BREAK_CALL calls from word 16 on, one lost NSYNC, a second run
        tile = dispersed_words(po, 4096, 0, seed)
        n_out = LONG_WORDS
        corpus, nerr = np.tile(tile, (n_out // 4096 + 1, 1))[:n_out], np.zeros(n_out, np.int32)
        _lost_nsync(po, corpus, [16 + 16 * LONG_BREAK_CALL], seed)
    elif kind == "cut":                                          # a piece of 700 words, clean, the NSYNC packets at the output words = arg (mod 8)
        n_out = 700
        corpus, nerr = dispersed_words(po, 704, int(arg), seed)[:n_out], np.zeros(n_out, np.int32)
    else:
        raise ValueError(name)
    case = {"name": name, "stream": viterbi_stream(po, corpus, seed), "n_out": n_out, "nerr": nerr, "corpus": corpus, "sent": sent}
    _cases[name] = case
    return case


def cut_hit(po, phase16, at):
    """the piece `cut-<phase16 % 8>` with the output word `at` replaced by garbage whose byte 0 is not the NSYNC"""
    base = outer_case(po, f"cut-{phase16 % 8}")
    corpus = base["corpus"].copy()
    corpus[at - JUNCTION] = np.random.RandomState(at).randint(0, 256, 204)
    corpus[at - JUNCTION, 0] = 0
    return viterbi_stream(po, corpus, sum(base["name"].encode()) + 1000)
