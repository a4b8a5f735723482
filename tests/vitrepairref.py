"""The check, repair and walk passes behind the HIP chunk decoders (k_viterbi3.hpp: viterbi_check_kernel, v3_repair_rows, v3_seq_walk, viterbi_fix_kernel), replayed on the
CPU with the oracle's decoder (oracle/o_viterbi.c) in the reference's own state representation: the 64 path metrics right behind a get_output call (lib/d_viterbi.c:728-732 has just
subtracted their minimum and cleared the path bytes).  Only o_viterbi_decode_snap and o_viterbi_decode_from are used.

  own[c]   state of chunk c's decoder (started W windows early from equal metrics) at its chunk's first window
  pred[c]  state there of the decoder whose bytes fill chunk c - 1
  check    the chunks with own[c] != pred[c]                                                                               -> listed
  repair   each of them decoded again from pred[c], own[c] = pred[c]; where the state it reaches at chunk c + 1 is not pred[c + 1]: fix[c + 1]   -> flagged
  walk     one decoder, in stream order over the flagged chunks: from fix[c] through chunk c, on through c + 1 unless it arrives in own[c + 1]

Positions.  get_output call j (counted from 1) stands behind trellis step 8 j - 2 and closes window j; output byte b is the path byte of window b + 2, so the decoder whose bytes
begin with byte b0 is in its "state at the chunk's first window" right behind call b0 + 1.  Chunk c's first byte is origin + c B.

Two placements:
  start="fresh"  the model tests/test_viterbi_repair_model.py has always run: origin = W - 1, chunk c's decoder is a fresh stream over the input from byte c B of the output on (its
                 first window has six steps, as a stream's has), chunk 0 is the streaming decoder over [0, B + W - 1)
  start="grid"   the kernels' placement: origin = 0, chunk c's decoder takes up the stream with all metrics equal right behind call b0 + 1 - W -- at the top of window b0 + 2 - W, where
                 viterbi3_kernel starts it (w0 = b0 + 2 - warm); a decoder that would start in front of the stream is the streaming decoder (the kernel feeds it erasures up to the
                 stream's first step, which leave equal metrics equal).  With B = 24 every call of the single block keeps this grid (a call's chunk 0 starts at a multiple of 24 with the
                 carried streaming state), so one Replay serves any cut into calls: launch(i0, i1) replays the passes over the chunks i0 .. i1 - 1 with chunk i0 streaming.

The unit is the smallest stretch of the stream that is whole in input bytes, output bytes, puncture periods and 16-bit output cadences (sub-streams are cut at units, so that the
depuncturer and the output cadence of a decoder over a sub-stream run as they do in the stream)."""
import ctypes as C

import numpy as np

# (m, k) -> (input bytes, output bytes) of a unit; k of the code rate k / (k + 1)
UNITS = {(4, 1): (8, 2), (6, 2): (4, 2), (2, 2): (12, 2), (2, 1): (16, 2), (6, 7): (32, 21)}


def lib(po):
    L = po.lib()
    L.o_viterbi_decode_snap.restype = C.c_size_t
    L.o_viterbi_decode_snap.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.o_viterbi_decode_from.restype = C.c_size_t
    L.o_viterbi_decode_from.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return L


class Replay:
    """the streaming decoder and the chunk decoders of one stream, once; launch() replays the passes over a range of chunks and leaves them unchanged"""

    def __init__(self, po, c, B, W, vin, start="grid", nch=None, nt=None):
        self.L, self.c, self.B, self.W, self.start = lib(po), c, B, W, start
        self.UI, self.UO = UNITS[(c.m, c.k)]
        assert len(vin) % self.UI == 0 and (start == "grid" or (start == "fresh" and B % self.UO == 0))   # (the grid placement cuts its sub-streams at the unit in front of a chunk: any B)
        self.vin = np.ascontiguousarray(vin, np.uint8)
        self.nt = nt = nt if nt is not None else {1: 5, 2: 9, 3: 10, 5: 15, 7: 24}[c.k]
        ncalls = len(vin) // self.UI * self.UO                                  # get_output calls of the whole stream
        self.origin = origin = 0 if start == "grid" else W - 1
        self.total_out = ncalls - nt
        self.nch = nch if nch is not None else -(-(self.total_out - origin) // B)   # the kernels' count: every chunk that has a byte
        n = self.nch
        # ---- the streaming decoder, and its state at every chunk's first window
        at = np.array([origin + i * B + 1 for i in range(1, n + 1)], np.int64)
        self.full = np.zeros(ncalls + 64, np.uint8)
        truth = np.zeros((n + 1, 64), np.uint8)
        self.nfull = self.L.o_viterbi_decode_snap(C.byref(c), self.vin.ctypes.data, len(self.vin), self.full.ctypes.data, at.ctypes.data, len(at), truth.ctypes.data)
        assert self.nfull == self.total_out
        self.truth = np.concatenate([np.zeros((1, 64), np.uint8), truth[:n]])   # truth[i]: behind call p(i) + 1, i >= 1 (the last chunks' successors may lie behind the stream's end)
        self.span = (2 * B + W + nt + 2 * self.UO) // self.UO + 2                # units a chunk decoder / a repair reads
        # ---- the chunk decoders i >= 1: own state, the state they leave for the next chunk, their bytes
        self.dec_own = np.zeros((n + 1, 64), np.uint8); self.dec_next = np.zeros((n + 1, 64), np.uint8)
        self.plain = self.full.copy()                                           # the plain chunk decoders' bytes (chunk 0: the streaming decoder's)
        self.streaming = np.zeros(n + 1, bool); self.streaming[0] = True       # chunks whose decoder IS the streaming decoder
        zeros = np.zeros(64, np.uint8)
        for i in range(1, n):
            p = origin + i * B
            if start == "grid" and p + 1 - W <= 0:
                self.streaming[i] = True; self.dec_own[i] = self.truth[i]; self.dec_next[i] = self.truth[i + 1]
                continue
            s2 = np.zeros((2, 64), np.uint8)
            if start == "fresh":
                u, sub = self._sub(i * B)
                o = np.zeros(len(sub) // self.UI * self.UO + 64, np.uint8)
                self.L.o_viterbi_decode_snap(C.byref(c), sub.ctypes.data, len(sub), o.ctypes.data, np.array([W, B + W], np.int64).ctypes.data, 2, s2.ctypes.data)
            else:
                u, sub = self._sub(p - W)
                o = np.zeros(len(sub) // self.UI * self.UO + 64, np.uint8)
                self.L.o_viterbi_decode_from(C.byref(c), sub.ctypes.data, len(sub), o.ctypes.data, p + 1 - W - u * self.UO, zeros.ctypes.data,
                                             np.array([p + 1 - u * self.UO, p + B + 1 - u * self.UO], np.int64).ctypes.data, 2, s2.ctypes.data)
            lo = p - u * self.UO
            self.plain[p:p + B] = o[lo:lo + B]
            self.dec_own[i] = s2[0]; self.dec_next[i] = s2[1]
        self.plain_wrong = int((self.plain[:self.nfull] != self.full[:self.nfull]).sum())

    def _sub(self, first_byte):
        """the sub-stream from the unit that holds output byte first_byte on: (its unit, the input)"""
        u = max(first_byte, 0) // self.UO
        return u, np.ascontiguousarray(self.vin[u * self.UI:(u + self.span) * self.UI])

    def _job(self, i, state, out):
        """decode chunk i from `state` at its first window: its bytes into out, the state at the next chunk's first window"""
        p = self.origin + i * self.B
        u, sub = self._sub(p)
        o = np.zeros(len(sub) // self.UI * self.UO + 64, np.uint8); e = np.zeros((1, 64), np.uint8)
        self.L.o_viterbi_decode_from(C.byref(self.c), sub.ctypes.data, len(sub), o.ctypes.data, p + 1 - u * self.UO, np.ascontiguousarray(state).ctypes.data,
                                     np.array([p + self.B + 1 - u * self.UO], np.int64).ctypes.data, 1, e.ctypes.data)
        lo = p - u * self.UO
        out[p:p + self.B] = o[lo:lo + self.B]
        return e[0].copy()

    def check(self, i0=0, i1=None):
        """the check alone: the chunks of i0 + 1 .. i1 - 1 whose own state is not their predecessor's (chunk i0 streaming)"""
        i1 = self.nch if i1 is None else min(i1, self.nch)
        return [i for i in range(i0 + 1, i1)
                if (self.dec_own[i] != (self.truth[i] if (i - 1 == i0 or self.streaming[i - 1]) else self.dec_next[i - 1])).any()]

    def launch(self, i0=0, i1=None):
        """the passes over the chunks i0 .. i1 - 1, chunk i0 being the streaming decoder (it starts the stream, or was handed its state).  Returns a dict: out (the assembled bytes,
        indexed like the stream's; valid in [first byte of chunk i0, min(first byte of chunk i1, total_out))), listed, flagged (lists of chunks), starts, walked, own, pred"""
        n = self.nch
        i1 = n if i1 is None else min(i1, n)
        B = self.B
        out = self.plain.copy()
        own = self.dec_own.copy(); pred = np.zeros_like(own); fix = np.zeros_like(own)
        own[i0] = self.truth[i0]
        if i0 == 0 and self.start == "fresh":
            out[:self.origin + B] = self.full[:self.origin + B]
        else:
            out[self.origin + i0 * B:self.origin + (i0 + 1) * B] = self.full[self.origin + i0 * B:self.origin + (i0 + 1) * B]
        for i in range(i0 + 1, i1 + 1):
            if i <= n:
                pred[i] = self.truth[i] if (i - 1 == i0 or self.streaming[i - 1]) else self.dec_next[i - 1]
        # ---- check
        listed = [i for i in range(i0 + 1, i1) if (own[i] != pred[i]).any()]
        # ---- repair (every listed chunk on its own: the order does not matter)
        flagged = np.zeros(n + 2, bool)
        for i in listed:
            own[i] = pred[i]
            end = self._job(i, pred[i], out)
            if i + 1 < i1 and (end != pred[i + 1]).any():
                fix[i + 1] = end; flagged[i + 1] = True
        nflagged = [int(i) for i in np.flatnonzero(flagged)]
        # ---- the walk
        pos, walked, starts = i0, 0, 0
        while True:
            nxt = [i for i in nflagged if i > pos]
            if not nxt:
                break
            i = nxt[0]; state = fix[i].copy(); starts += 1
            while True:
                own[i] = state; pred[i] = state
                end = self._job(i, state, out); walked += 1
                if i + 1 >= i1:
                    pos = i1; break
                eq = (end == own[i + 1]).all()
                pred[i + 1] = end
                if eq:
                    pos = i + 1; break
                i += 1; state = end
        return dict(out=out, listed=listed, flagged=nflagged, starts=starts, walked=walked, own=own, pred=pred, i0=i0, i1=i1)


def garbage(c, seed, nbytes_in):
    """uniform random decoder symbols: what the decoder sees of a channel that carries nothing"""
    return np.random.RandomState(seed).randint(0, 1 << c.m, nbytes_in).astype(np.uint8)


# ---- the inputs of tests/test_gpu_viterbi_handover.py, certified by tests/test_viterbi_handover_model.py: garbage through the single block at bsize 48, chunks of 24 bytes, warm-up 48,
# 288 KB decoded.  name -> (constellation, code rate, seed, what the walk does on it).  Each seed is the first of 1, 2, 3, ... that meets its case's conditions in the model test.
BSIZE, CHUNK, WARM, DECODED = 48, 24, 48, 288000
INPUTS = {"qam64-2/3-continuation": (2, 1, 1, "continuation"), "qam64-2/3-absorption": (2, 1, 5, "absorption"), "qpsk-2/3-continuation": (0, 1, 1, "continuation"),
          "qam16-1/2": (1, 0, 1, None), "qam64-7/8": (2, 4, 1, None)}
NTB = (5, 9, 10, 15, 24)
_cache = {}


def block_sizes(c):
    """(input bytes, output bytes) of one reference block at BSIZE"""
    return BSIZE * c.n // c.m, BSIZE * c.k // 8


def stream(po, const, cr, seed, decoded=DECODED):
    c = po.cfg(const, cr, po.T2k)
    d_nsym, d_nout = block_sizes(c)
    nblocks = -(-decoded // d_nout)
    return c, nblocks, garbage(c, seed, nblocks * d_nsym)


def replay(po, name):
    """(cfg, reference blocks, decoder input, Replay, its one-launch result) of a named input, computed once per process and left unchanged"""
    if name not in _cache:
        const, cr, seed, _ = INPUTS[name]
        c, nblocks, vin = stream(po, const, cr, seed)
        R = Replay(po, c, CHUNK, WARM, vin)
        _cache[name] = (c, nblocks, vin, R, R.launch())
    return _cache[name]


def call_grid(nt, d_nout, calls, B=CHUNK):
    """the single block's launches (dvbt_blocks.inc, viterbi_call) for calls of calls[i] reference blocks behind a reset: a list of (grid0, out_lo, out_hi, chunks) per call, None for
    a call that produces nothing.  grid0: where the carried state stands, the first byte of the call's chunk 0"""
    steps8, have, grid0, res = 0, False, 0, []
    for nb in calls:
        out_lo = max(steps8 - nt, 0)
        steps8 += nb * d_nout
        out_hi = max(steps8 - nt, 0)
        if out_hi <= out_lo:
            res.append(None); continue
        g0 = grid0 if have else 0
        chunks = -(-(out_hi - g0) // B)
        b0_last = g0 + (chunks - 1) * B
        grid0 = b0_last + (out_hi - b0_last) // 24 * 24; have = True
        res.append((g0, out_lo, out_hi, chunks))
    return res


FIX_SMALL = 1024                       # k_viterbi3.hpp, V3_FIX_SMALL: launches of at most this many chunks run check, repair and walk as one workgroup (viterbi_fix_kernel)


def fused_blocks(c):
    """reference blocks per call such that every call of a stream is a launch of at most FIX_SMALL chunks: the carried state stands up to 23 bytes in front of a call's first byte,
    so a call of exactly FIX_SMALL chunks' worth of bytes can span FIX_SMALL + 1 chunks of the grid; this is the largest call that never does (1023 or 1024 chunks per launch)"""
    return (FIX_SMALL * CHUNK - (CHUNK - 1)) // block_sizes(c)[1]


def cut(nblocks, per_call):
    """the stream in calls of per_call[i] blocks, the pattern repeating"""
    calls, k = [], 0
    while sum(calls) < nblocks:
        calls.append(min(per_call[k % len(per_call)], nblocks - sum(calls))); k += 1
    return calls


def launches(po, name, calls):
    """per call of the named input cut into `calls`: None, or (grid entry, first chunk, end chunk) of its launch on the 24-byte grid"""
    c, nblocks, vin, R, _ = replay(po, name)
    res = []
    for g in call_grid(R.nt, block_sizes(c)[1], calls):
        res.append(None if g is None else (g, g[0] // CHUNK, g[0] // CHUNK + g[3]))
    return res


def fused_call_above_20(po):
    """(input, call) of the first fused launch, over INPUTS in order, whose check lists more than 20 chunks"""
    for name in INPUTS:
        c, nblocks, vin, R, _ = replay(po, name)
        for k, l in enumerate(launches(po, name, cut(nblocks, [fused_blocks(c)]))):
            if l is not None and len(R.check(l[1], l[2])) > 20:
                return name, k
    return None, -1
