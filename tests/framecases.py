"""Streams for tests/test_gpu_frames.py (and the CPU checks of tests/test_frameref.py): what the symbol kernels would leave behind for the frame bookkeeping and the
inner stage -- a pattern index and the equalised TPS carriers per symbol, label bytes -- built from a transmitted TPS bit stream and a list of the true symbols that
arrive.  A clean stream is the symbols t0, t0 + 1, ...; the cases below drop, repeat and mislabel symbols, corrupt TPS words and set traps for the sync-word match.
Nothing here knows what the kernels make of a stream: the expectation is frameref's."""
import bisect

import numpy as np

import frameref as fr

N_TPS = {0: 17, 1: 68}                                              # TPS carriers per mode (2k, 8k)
SEG, WARM, WG = 32, 204, 8192                                       # the parallel pass's lane, warm-up and workgroup, in symbols (to place the cases; the model knows none of them)
CELL = {40: 1, 43: 1, 46: 1}                                        # default parameters of a word: some bits of s40..s47 set


def word(g, fields=None):
    """the word frame g (global frame number) transmits by default"""
    f = dict(CELL)
    f.update(fields or {})
    return fr.tps_word(g % 4, f)


class Stream:
    """ts: the true symbols (global numbers: frame g = t // 68, position l = t % 68) in arrival order.  words: {g: 68 bits} replacing the default word of a frame
    (as transmitted: a corrupted word is given corrupted).  mod_off: {arrival index: offset added to the pattern index}.  vote0: {g: +1 / -1} fixes the sign of the
    vote at symbol 0 of frame g (default: what the transmitter's restart of the DBPSK from the reference sequence gives -- the parity of the previous word)."""

    def __init__(self, ts, words=None, mod_off=None, vote0=None, mode=0, seed=1, default=word):
        self.ts = np.asarray(list(ts), np.int64)
        self.words, self.mod_off, self.vote0, self.mode, self.seed, self.default = dict(words or {}), dict(mod_off or {}), dict(vote0 or {}), mode, seed, default
        self.n = len(self.ts)
        self.dirty_frames = set(self.words) | set(self.vote0)
        self._build()

    def bits(self, g):
        return self.words[g] if g in self.words else self.default(g)

    def _build(self):
        n_tps = N_TPS[self.mode]
        self.mods = (self.ts % 4).astype(np.int32)
        for i, d in self.mod_off.items():
            self.mods[i] = (self.mods[i] + d) % 4
        if self.n == 0:
            self.tps = np.zeros((0, n_tps), np.complex64)
            return
        g0, g1 = int(self.ts.min()) // 68, int(self.ts.max()) // 68
        sign = np.empty((g1 - g0 + 1) * 68)
        last = 1.0
        for g in range(g0, g1 + 1):
            b = np.asarray(self.bits(g), np.int64)
            first = last * self.vote0[g] if g in self.vote0 else 1.0  # symbol 0 restarts from the reference sequence
            sign[(g - g0) * 68:(g - g0 + 1) * 68] = first * np.cumprod(np.concatenate([[1], 1 - 2 * b[1:]]))
            last = sign[(g - g0 + 1) * 68 - 1]
        rng = np.random.RandomState(self.seed)
        phi = rng.uniform(-np.pi, np.pi, n_tps)
        amp = rng.uniform(0.5, 1.5, (self.n, n_tps))
        jit = rng.uniform(-0.3, 0.3, (self.n, n_tps))                  # two symbols differ by at most 0.6 rad: cos >= 0.82, far from the vote's boundary
        self.tps = (amp * sign[self.ts - g0 * 68][:, None] * np.exp(1j * (phi[None, :] + jit))).astype(np.complex64)


def clean(n, t0=0, **kw):
    return Stream(range(t0, t0 + n), **kw)


def wrong_index(n, pos, d, t0=0, **kw):
    return Stream(range(t0, t0 + n), mod_off={pos: d}, **kw)


def dropped(n, pos, t0=0, **kw):
    return Stream([t for t in range(t0, t0 + n + 1) if t != t0 + pos], **kw)


def repeated(n, pos, t0=0, **kw):
    ts = list(range(t0, t0 + n - 1))
    return Stream(ts[:pos] + [ts[pos - 1]] + ts[pos:], **kw)


def flipped(g, bit, fields=None):
    w = list(word(g, fields))
    w[bit] ^= 1
    return w


def bad_frames(n, frames, t0=0, bit=30, **kw):
    """the frames `frames` arrive with one wrong bit each"""
    return Stream(range(t0, t0 + n), words={g: flipped(g, bit) for g in frames}, **kw)


def sync_wrong(g, i, reparity=True):
    """frame g with s_i of its sync word wrong; reparity: the parity is that of the word as sent (the word is a code word, only no sync word)"""
    base = fr.SYNC_EVEN if g % 2 == 0 else fr.SYNC_ODD
    s = list(base)
    s[i - 1] ^= 1
    if reparity:
        return fr.tps_word(g % 4, CELL, sync=s)
    w = list(word(g))
    w[i] ^= 1
    return w


def embedded_sync(g, sync_bit=None):
    """a code word whose s33..s47 are the first fifteen bits of the even sync word: where the FIFO is not cleared at the word's end its bits 1..15 match 32 symbols
    behind it.  sync_bit: that bit of the word's own sync word is wrong (in front of the parity's computation), so its end is no frame end"""
    f = dict(CELL)
    f.update({33 + j: fr.SYNC_EVEN[j] for j in range(15)})
    s = list(fr.SYNC_EVEN if g % 2 == 0 else fr.SYNC_ODD)
    if sync_bit is not None:
        s[sync_bit - 1] ^= 1
    return fr.tps_word(g % 4, f, sync=s)


def cell_words(a=0x5A, b=0xC3):
    """a broadcast's frames: s40..s47 carry one half of the cell id in frames 0 and 2, the other in frames 1 and 3"""
    def w(g):
        v = a if g % 2 == 0 else b
        return fr.tps_word(g % 4, {40 + j: (v >> (7 - j)) & 1 for j in range(8)})
    return w


def locked_state(t0, fi_start=3):
    """the members a chain in stable lock holds in front of true symbol t0, for a hunt that wants frame number fi_start in front of a superframe start (the FIFO is
    left empty: state_after gives one that is partly filled)"""
    q = t0 % 272
    return fr.State(None, (q - 1) % 68, 1, (fi_start + q // 68) % 4, (t0 - 1) % 4, 0)


def state_after(stream, k, **kw):
    """the model's members after the first k symbols of `stream` (a partly filled FIFO, known counters), and the carriers of symbol k - 1"""
    st = fr.State()
    maj = fr.vote(stream.tps[:k])
    fr.bookkeeping(stream.mods, maj, k, st, **kw)
    return st, stream.tps[k - 1].copy()


def tail(stream, k):
    """the stream from its symbol k on"""
    s = Stream.__new__(Stream)
    s.__dict__.update(stream.__dict__)
    s.ts, s.mods, s.tps, s.n = stream.ts[k:], stream.mods[k:], stream.tps[k:], stream.n - k
    s.mod_off = {i - k: d for i, d in stream.mod_off.items() if i >= k}
    return s


# ---------------------------------------------------------------- the parallel pass's sufficient condition, from the stream
def lanes_off(stream, ntot, exp, quick=True):
    """The design: a lane takes SEG symbols and starts WARM symbols early from blank members; where its warm-up holds an intact frame end it reaches its own segment
    with the sequential members, and when every lane does, all neighbours agree and no fallback is needed.  Returns the first symbols of the lanes for which that
    does NOT hold: the members of the model, started blank WARM symbols early, differ in front of the lane from those of the sequential run (exp: frameref.run's
    result with snap_every = SEG).  A lane whose warm-up begins at symbol 0 starts from the true members.  The first lane listed has a neighbour that is right, so a
    non-empty list means the neighbours disagree.  quick: a lane whose warm-up holds a whole undisturbed frame, and one symbol in front, that the sequential run
    found valid is taken as right without running the model (tests/test_frameref.py checks that this changes nothing)."""
    ends = sorted(s for s, _ in exp["valid"])
    dirty = _dirty_symbols(stream)
    off = []
    for s0 in range(0, ntot, SEG):
        sw = s0 - WARM
        if sw <= 0:
            continue
        if quick and any(not dirty[e - 68:s0].any() for e in ends[bisect.bisect_left(ends, sw + 68):bisect.bisect_left(ends, s0)]):
            continue
        st = fr.State()
        fr.bookkeeping(stream.mods[sw:s0], exp["maj"][sw:s0], s0 - sw, st)
        if st.members()[:6] != exp["snaps"][s0][:6]:
            off.append(s0)
    return off


def _dirty_symbols(stream):
    """arrival positions at which the stream is not the clean one with default words"""
    d = np.zeros(stream.n + 1, bool)
    if stream.n:
        d[1:stream.n] = np.diff(stream.ts) != 1
        for i in stream.mod_off:
            d[i] = True
            if i + 1 <= stream.n:
                d[i + 1] = True
        for g in stream.dirty_frames:
            d[:stream.n] |= (stream.ts // 68 == g) | (stream.ts // 68 == g + 1)     # (a word's parity decides the sign that the next frame starts from)
        if stream.default is not word:
            d[:] = True
    return d


# ---------------------------------------------------------------- labels
_LABELS = {}


def labels(n, payload, m, seed=7):
    """n rows of random label bytes below 2^m: one array per (payload, m), generated in blocks of 1024 rows of their own seed, so that a longer array begins with the
    shorter one; rows shared by every case"""
    key = (payload, m, seed)
    have = _LABELS.get(key)
    if have is None or len(have) < n:
        nb = (max(n, 720) + 1023) // 1024
        have = np.concatenate([np.random.RandomState(seed + 7919 * b).randint(0, 1 << m, size=(1024, payload), dtype=np.uint8) for b in range(nb)])
        _LABELS[key] = have
    return have[:n]


# ---------------------------------------------------------------- vote inputs
def _vote_try(n, n_tps, seed, tie, zeros, nan_row, prev0):
    rng = np.random.RandomState(seed)
    # row r is v[r + 1]; its phase step from the row in front lies at least 0.2 rad from +-pi/2
    step = rng.uniform(0.2, np.pi / 2 - 0.2, (n + 1, n_tps)) * rng.choice([-1, 1], (n + 1, n_tps)) + np.pi * rng.randint(0, 2, (n + 1, n_tps))
    if tie is not None:
        step[tie + 1] = rng.uniform(-1.0, 1.0, n_tps) + np.where(np.arange(n_tps) % 2 == 0, 0.0, np.pi)      # half the carriers in phase, half opposed
    ph = np.cumsum(step, 0) + rng.uniform(-np.pi, np.pi, n_tps)[None, :]
    amp = rng.uniform(0.25, 4.0, (n + 1, n_tps)) * 10.0 ** rng.randint(-3, 4, (n + 1, 1))
    v = (amp * np.exp(1j * ph)).astype(np.complex64)
    rows, p0 = v[1:].copy(), (v[0].copy() if prev0 else None)
    if zeros is not None:
        r, items = zeros
        for k, kind in items:
            pv = rows[r - 1, k] if r > 0 else p0[k]
            if kind == "cancel":                                       # v = 2i pv: the two products are exact negatives of each other in any precision -> +0
                rows[r, k] = np.complex64(complex(-2.0 * float(pv.imag), 2.0 * float(pv.real)))
            elif kind == "+0":                                         # both products +0
                rows[r, k] = np.complex64(complex(0.0 if pv.real > 0 else -0.0, 0.0 if pv.imag > 0 else -0.0))
            else:                                                      # both products -0
                rows[r, k] = np.complex64(complex(-0.0 if pv.real > 0 else 0.0, -0.0 if pv.imag > 0 else 0.0))
    if nan_row is not None:
        rows[nan_row] = np.complex64(complex(np.nan, np.nan))
    re, _ = fr.vote_re(rows, p0)
    with np.errstate(invalid="ignore"):
        crafted = ~np.isfinite(re) | (re == 0)
    return rows, p0, crafted


def vote_case(n, n_tps, seed, tie=None, zeros=None, nan_row=None, prev0=False):
    """rows cfloat[n][n_tps] of random amplitudes (seven decades) and phases, prev0 or None, and the mask of the carriers whose product is exactly zero or NaN by
    construction.  tie: a row whose carriers split evenly between the two signs.  zeros: (row, [(carrier, "cancel" | "+0" | "-0")]).  nan_row: a row of NaNs.
    Every other carrier meets frameref.vote_margin_ok's condition: the generator takes the next seed until it does."""
    for k in range(64):
        rows, p0, crafted = _vote_try(n, n_tps, seed + 1000 * k, tie, zeros, nan_row, prev0)
        want = np.zeros_like(crafted)
        if p0 is None and n:
            want[0] = True                                             # against zeros
        if zeros is not None:
            for c, kind in zeros[1]:
                want[zeros[0], c] = True
                if kind != "cancel" and zeros[0] + 1 < n:
                    want[zeros[0] + 1, c] = True                      # a zero carrier makes the next symbol's product zero too
        if nan_row is not None:
            want[nan_row] = True
            if nan_row + 1 < n:
                want[nan_row + 1] = True
        if (crafted == want).all() and fr.vote_margin_ok(rows, p0, crafted):
            return rows, p0, crafted
    raise AssertionError("no seed gives the margin")


# ---------------------------------------------------------------- the disturbed streams of tests/test_gpu_frames.py (tests/test_frameref.py walks them on the CPU)
# a lane's first symbol and the symbols around it, the first symbol of a lane's warm-up (lane 10: 320 - 204), the last and the first symbol of a frame (the streams
# begin at a frame's first symbol), the last symbol of the first workgroup and the first of the second
PLACES = (31, 32, 33, 116, 339, 340, 8191, 8192)
KINDS = ("+1", "+2", "+3", "drop", "repeat")
BAD = {"one": (0,), "two": (0, 1), "four": (0, 1, 2, 3), "six": tuple(range(6))}
BAD_PLACES = ("start", "middle", "8192")


def disturbed(kind, pos):
    n = 700 if pos < 600 else 8500
    if kind[0] == "+":
        return wrong_index(n, pos, int(kind[1]))
    return dropped(n, pos) if kind == "drop" else repeated(n, pos)


def bad_words(kind, place):
    """frames with a flipped TPS bit: one, two, four and six in a row, near the stream's start, in its middle and across symbol 8192"""
    g0, n = {"start": (1, 700), "middle": (4, 700), "8192": (8192 // 68 - len(BAD[kind]) // 2, 8700)}[place]
    return bad_frames(n, [g0 + j for j in BAD[kind]], bit=30 + len(kind))


def fallback_length(n):
    """five corrupted words in a row early in a stream of n symbols"""
    return bad_frames(n, range(6, 11), t0=11)
