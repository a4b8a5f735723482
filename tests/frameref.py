"""A model of the launches between the symbol kernels and the Viterbi decoder (tps_vote_kernel, tps_fsm_par_kernel, tps_tail_kernel, inner_kernel<6>), in plain
Python / numpy, written from the reference's statements and not from the kernels: the DBPSK majority vote (reference_signals_impl.cc:929-945), the pilot
engine's symbol / frame bookkeeping (parse_input :1228-1241, process_tps_data :952-1028 with verify_bch_code :385-425), the demodulator's superframe hunt
(demod_reference_signals_impl.cc:73-77,108-143), the sizes of the stages behind (viterbi_decoder_impl.cc:141-153,198,310; convolutional_deinterleaver's
set_output_multiple(2)) and, through the oracle's primitives, the two inner de-interleavers.  One symbol at a time, a 68-element list as the FIFO, the bit-serial
LFSR as the BCH check: nothing of the segment-parallel scheme, the byte table or the three-word FIFO of k_frontend.hpp.  tests/test_frameref.py pins it to the oracle."""
import ctypes as C

import numpy as np

SYNC_EVEN = [0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 0]        # s1..s16 of frames 0 and 2 (reference_signals_impl.cc:54-60); frames 1 and 3 carry the complement
SYNC_ODD = [1 - b for b in SYNC_EVEN]
NTRACEBACK = (5, 9, 10, 15, 24)                                      # viterbi_decoder_impl.cc:95-124, by code rate
STATIC_BITS = [i for i in range(17, 54) if i not in (23, 24)]        # what every frame of a stream repeats: length indicator s17-s22, parameters s25-s53
NO_CAND = 0x7fffffff


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- BCH (verify_bch_code / generate_bch_code)
def _lfsr(bits53):
    reg = 0
    for d in [0] * 60 + list(bits53):
        fb = 1 & (d ^ reg)
        reg >>= 1
        reg |= fb << 13
        reg ^= (fb << 12) ^ (fb << 11) ^ (fb << 9) ^ (fb << 8) ^ (fb << 7) ^ (fb << 5) ^ (fb << 4)
    return reg


def bch_check(w68):
    """0 when bits 54..67 are the parity of bits 1..53, else -1"""
    reg = _lfsr([int(b) for b in w68[1:54]])
    for i in range(14):
        if int(w68[54 + i]) != (1 & (reg >> i)):
            return -1
    return 0


def tps_word(frame, fields=None, sync=None, frame_bits=None):
    """a BCH-valid 68-bit TPS frame: s0 = 0, s1..s16 the sync word of `frame`'s parity (or `sync`, 16 bits), s23 s24 the frame number (or `frame_bits`), s17..s53
    from `fields` {bit: value} (default 0, the length indicator 010111 as the reference sends it), s54..s67 the parity"""
    w = [0] * 68
    w[1:17] = list(sync) if sync is not None else (SYNC_EVEN if frame % 2 == 0 else SYNC_ODD)
    w[17:23] = [0, 1, 0, 1, 1, 1]
    fb = frame_bits if frame_bits is not None else ((frame >> 1) & 1, frame & 1)
    for i, v in (fields or {}).items():
        assert 17 <= i <= 53
        w[i] = int(v)
    w[23], w[24] = int(fb[0]), int(fb[1])
    reg = _lfsr(w[1:54])
    for i in range(14):
        w[54 + i] = 1 & (reg >> i)
    return w


def static_word(w68):
    """the 64-bit word the state block reports for a valid frame: bit i = s_i for the static bits, bit 63 set"""
    v = 1 << 63
    for i in STATIC_BITS:
        v |= int(w68[i]) << i
    return v


# ---------------------------------------------------------------- DBPSK majority vote
def vote_re(tps, prev0=None):
    """re[s][k] = Re(v conj(pv)) in float64 from the float32 inputs; the symbol in front of symbol 0 is prev0 or zeros"""
    v = np.asarray(tps, np.complex64)
    n, k = v.shape
    p0 = np.zeros(k, np.complex64) if prev0 is None else np.asarray(prev0, np.complex64)
    pv = np.concatenate([p0[None, :], v[:-1]], 0) if n else v
    vx, vy, px, py = (a.astype(np.float64) for a in (v.real, v.imag, pv.real, pv.imag))
    return vx * px + vy * py, np.abs(vx * px) + np.abs(vy * py)


def vote(tps, prev0=None):
    """+1 per carrier with re >= 0, else -1 (a NaN counts -1)"""
    re, _ = vote_re(tps, prev0)
    with np.errstate(invalid="ignore"):
        return np.where(re >= 0, 1, -1).sum(1).astype(np.int64)


def vote_margin_ok(tps, prev0=None, crafted=None):
    """the GPU test's precondition: |re| > 2^-20 (|v.x pv.x| + |v.y pv.y|) for every carrier -- sixteen float32 roundings of the two-term sum, where the kernel's
    three roundings cost at most 2^-23 of it -- except the carriers marked `crafted`, whose re must be exactly zero or not a number (decided by no rounding)"""
    re, mag = vote_re(tps, prev0)
    crafted = np.zeros(re.shape, bool) if crafted is None else np.asarray(crafted, bool)
    with np.errstate(invalid="ignore"):
        ok = np.abs(re) > mag * 2.0 ** -20
        exact = ~np.isfinite(re) | (re == 0)
    return bool((ok | crafted).all() and exact[crafted].all())


# ---------------------------------------------------------------- bookkeeping
class State:
    """members of pilot_gen (d_rcv_tps_data, d_symbol_index, d_symbol_index_known, d_frame_index, the pattern index of the previous symbol) and of the demodulator (d_init)"""

    def __init__(self, fifo=None, symbol_index=0, symbol_index_known=0, frame_index=0, prev_mod=0, d_init=0):
        self.fifo = list(fifo) if fifo is not None else [0] * 68
        assert len(self.fifo) == 68
        self.symbol_index, self.symbol_index_known, self.frame_index, self.prev_mod, self.d_init = symbol_index, symbol_index_known, frame_index, prev_mod, d_init

    def copy(self):
        return State(self.fifo, self.symbol_index, self.symbol_index_known, self.frame_index, self.prev_mod, self.d_init)

    def members(self):
        lo = sum(int(b) << i for i, b in enumerate(self.fifo[:64]))
        hi = sum(int(b) << i for i, b in enumerate(self.fifo[64:]))
        return (lo, hi, self.symbol_index, self.symbol_index_known, self.frame_index, self.prev_mod, self.d_init)


def fi_start_of(constellation, mode):
    """demod_reference_signals_impl.cc:73-77"""
    return 2 if (constellation == 2 and mode == 1) else 3


def cut_hunt(fi_start, start_delay_symbols):
    """dvbt_rx_cut.start_delay_symbols: the hunt fires that many symbols behind a superframe start -> (si_start, fi_start, hunt_known)"""
    return start_delay_symbols % 68, (fi_start + start_delay_symbols // 68) % 4, 1 if start_delay_symbols > 0 else 0


def bookkeeping(mods, maj, ntot, st, si_start=0, fi_start=3, hunt_known=0, restart_hunt=False, snap_every=0, snaps=None):
    """ntot symbols through parse_input / process_tps_data and the superframe hunt, from the members `st` (changed in place).  Returns sym_index[ntot], the flags
    (0 dropped, 1 produced, 2 produced and superframe start), first_out (-1: none), the words of the valid frames as (symbol, 68 bits).  snap_every > 0: snaps[s] = the members in front of symbol s, for every s that is a multiple of it"""
    if restart_hunt:
        st.d_init = 0                                                  # the sync_start tag on the period's first item (:115-116)
    sym_index, flags, valid, first_out = [], [], [], -1
    for s in range(ntot):
        if snap_every and s % snap_every == 0:
            snaps[s] = st.members()
        mod = int(mods[s])
        diff = (mod - st.prev_mod + 4) % 4                             # process_spilot_data's return value
        st.prev_mod = mod
        st.symbol_index = (st.symbol_index + diff) % 68                # :1228
        si, fi = st.symbol_index, st.frame_index                       # :1231-1233, what the demodulator sees
        for _ in range(diff):                                          # :955-970
            st.fifo.pop(0)
            if (not st.symbol_index_known) or st.symbol_index != 0:
                st.fifo.append(0 if maj[s] >= 0 else 1)
            else:
                st.fifo.append(0)
        end_frame = 0
        if st.fifo[1:16] == SYNC_EVEN[:15] or st.fifo[1:16] == SYNC_ODD[:15]:     # std::equal over begin() + 1 .. begin() + 16 (:973, :1000)
            if bch_check(st.fifo) == 0:
                st.frame_index = (st.fifo[23] << 1) | st.fifo[24]
                st.symbol_index_known = 1
                end_frame = 1
                valid.append((s, list(st.fifo)))
            else:
                st.symbol_index_known = 0
            st.fifo = [0] * 68
        if end_frame:
            st.symbol_index = 67                                       # :1240-1241
        sf = 0
        if not st.d_init:                                              # demod_reference_signals_impl.cc:118-136 (hunt_known: a piece on a shifted grid waits for set counters)
            if (si % 68) == si_start and (fi % 4) == fi_start and ((not hunt_known) or st.symbol_index_known):
                st.d_init = 1
                sf = 1
                if first_out < 0:
                    first_out = s
        sym_index.append(si)
        flags.append((2 if sf else 1) if st.d_init else 0)
    return np.array(sym_index, np.int64), np.array(flags, np.int64), first_out, valid


# ---------------------------------------------------------------- sizes behind the inner stage
def sizes(payload, m, k, n, code_rate, n_out_symbols, sym_off=0, bsize=768):
    """what a chain over the whole stream, whose first superframe start lies sym_off symbols in front of this period's, lets the period's stages touch.  The decoder
    works in blocks of bsize k decoded bits = bsize n / m input bytes (:141-153) and takes whole blocks of what has arrived (:198); its output lags ntraceback bytes
    (:277-279,310); the byte de-interleaver hands on pairs of items of 1632 bytes."""
    blk_in, blk_bits = bsize * n // m, k * bsize
    ibits = payload * m * k // n                                       # decoded bits per OFDM symbol
    nblocks = (sym_off + n_out_symbols) * payload // blk_in            # blocks of the whole stream up to this period's end
    nin = nblocks * blk_in - sym_off * payload
    steps = nblocks * blk_bits - sym_off * ibits
    clamp_in = nin < 0 or steps < 0
    if clamp_in:
        nin = steps = 0
    ntb = NTRACEBACK[code_rate]
    nb_g = nblocks * blk_bits // 8 - ntb
    clamp_g = nb_g < 0
    nb_g = max(nb_g, 0)
    nb = max(steps // 8 - ntb, 0)
    items_g = nb_g // 1632
    items_g -= items_g % 2
    words = items_g * 8 - sym_off * ibits // (8 * 204)
    clamp_w = words < 0
    words = max(words, 0)
    return {"n_vit_in": nin, "n_vit_steps": steps, "n_vit_bytes": nb, "stream_rs_items": items_g, "n_rs_words": words, "n_rs_items": words // 8, "sym_off": sym_off,
            "clamps": (clamp_in, clamp_g, clamp_w)}


# ---------------------------------------------------------------- inner stage (the oracle's primitives)
class Inner:
    def __init__(self, po, c):
        self.po, self.c, self.L = po, c, po.lib()
        self.h = np.zeros(c.payload, np.int32)
        self.L.o_sym_H(C.byref(c), _p(self.h))

    def rows(self, labels, sym_index):
        """symbol de-interleaver (parity of sym_index) then bit de-interleaver of each row -> (tap, hp / the output, lp or None)"""
        c, L = self.c, self.L
        labels = np.ascontiguousarray(labels, np.uint8)
        n = len(labels)
        tap = np.zeros_like(labels)
        for u in range(n):
            L.o_sym_interleave(C.byref(c), _p(self.h), _p(labels[u]), _p(tap[u]), int(sym_index[u]), 0)
        out = np.zeros_like(tap)
        lp = None
        if n:
            if c.hierarchy:
                lp = np.zeros_like(tap)
                L.o_bit_deinterleave_hier(C.byref(c), _p(tap), _p(out), _p(lp), C.c_size_t(tap.size))
            else:
                L.o_bit_deinterleave(C.byref(c), _p(tap), _p(out), C.c_size_t(tap.size))
        return tap, out, lp


# ---------------------------------------------------------------- the launches as a whole
def run(mods, tps, n_symbols, keep_last, constellation, mode, code_rate, payload, m, k, n, prev0=None, init=None, carried=None, sym_off=0, start_delay_symbols=0, bsize=768, snap_every=0):
    """the expected results of one call.  init: State in front of symbol 0 (fresh period from known members); prev0: continuation (hunt restarted, members =
    init or `carried`, the State the previous call left)"""
    ntot = n_symbols if keep_last else max(n_symbols - 1, 0)
    maj = vote(np.asarray(tps)[:n_symbols], prev0)
    if prev0 is not None:
        st = (init if init is not None else carried).copy()
    else:
        st = init.copy() if init is not None else State()
        st.d_init = 0                                                  # a fresh period hunts from the beginning
    si_start, fi_start, hunt_known = cut_hunt(fi_start_of(constellation, mode), start_delay_symbols)
    snaps = {}
    sym_index, flags, first_out, valid = bookkeeping(mods, maj, ntot, st, si_start, fi_start, hunt_known, restart_hunt=prev0 is not None, snap_every=snap_every, snaps=snaps)
    nout = ntot - first_out if first_out >= 0 else 0
    r = {"ntot": ntot, "maj": maj[:ntot], "sym_index": sym_index, "flags": flags, "first_out": first_out, "n_out_symbols": nout, "no_start": first_out < 0,
         "tps_bits": static_word(valid[-1][1]) if valid else 0, "valid": valid, "state": st, "snaps": snaps}
    r.update(sizes(payload, m, k, n, code_rate, nout, sym_off, bsize))
    return r
