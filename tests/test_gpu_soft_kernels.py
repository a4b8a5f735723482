"""The two soft-decision kernels ALONE (dvbt_debug_soft_viterbi, dvbt_debug_soft_demap: test hooks of the library), where tests/test_gpu_soft.py reaches them only
through the whole chain on a few superframes: the decoder at every chunk size on both sides of every change of its traceback segment length, with a task loop
that iterates (one workgroup, three passes, a last task with idle decoders, a clipped last chunk), at every code rate, on inputs no channel produces (all ties,
saturated values, erasure bursts, a stream that ends early), on streams shorter than a chunk; the demapper on decision boundaries, capped and vanishing channel
weights.  The decoder's reference is the model oracle/o_soft.c::o_soft_viterbi at the same B and nsteps (tests/test_soft_plan_model.py ties those to what a
segment plans): every byte of [0, total_out) equal, every byte behind still the 0xA5 the hook filled the buffer with.  The demapper's references are the model
o_soft_demap (identical), the formula in float64 (within the rounding) and -- for WHERE a soft value lands, on which the model shares its formula with the
kernel -- the oracle's hard chain demap -> symbol de-interleaver -> bit de-interleaver on the same carriers (the signs)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QPSK, T2k = 0, 0
NTB = {0: 5, 1: 9, 2: 10, 3: 15, 4: 24}
RATE_IDS = {0: "1/2", 1: "2/3", 2: "3/4", 3: "5/6", 4: "7/8"}
SIZES = (64, 94, 95, 142, 143, 190, 191, 238, 239, 286, 287, 304)      # both sides of every change of S = ceil((B + 2) / 48) * 6, and the ends of the range
S4_MAXSTEPS = 2928
# noise on the +-8 stream, per rate, chosen on the CPU so that the MODEL's output differs from the message in more than 0 and fewer than 12 % of the bits at every
# chunk size (asserted where the streams are used; 0.5 .. 6 % measured): the decoder has decisions to make and the comparison is not of two garbage streams
SIGMA = {0: 6.5, 1: 5.5, 2: 5.0, 3: 4.5, 4: 4.0}


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    L = gr_dvbt_amd.lib()
    L.dvbt_debug_soft_viterbi.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.dvbt_debug_soft_demap.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return gr_dvbt_amd


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def nsteps_for(B, cr):
    return -(-(256 + 8 * B + max(8 * NTB[cr], 128)) // 48) * 48


def total_for(B):
    """with ONE workgroup (4 wavefronts x 4 decoders): two full passes of the task loop, a third whose second task has idle decoders, a clipped last chunk"""
    return 16 * B * 2 + 4 * B + B // 3 + 1


def puncture(po, cr):
    po.lib().o_vit_puncture.restype = C.POINTER(C.c_ubyte)
    n = C.c_int()
    p = po.lib().o_vit_puncture(cr, C.byref(n))
    return np.array([p[i] for i in range(n.value)], np.uint8)


def encode(po, cr, msg):
    """the K = 7 encoder on the bits of msg (byte MSB = first step): r = state | b << 6, X = parity(r & 0x79), Y = parity(r & 0x5b), state = r >> 1; X, Y
    alternate, the rate's puncture pattern drops coded bits.  Returns the kept coded bits."""
    b = np.unpackbits(np.asarray(msg, np.uint8)).astype(np.uint8)
    h = np.concatenate([np.zeros(6, np.uint8), b])                    # h[t + 6 - d] = the bit d steps before step t = bit 6 - d of r
    d = lambda k: h[6 - k:len(h) - k]
    x = d(0) ^ d(1) ^ d(2) ^ d(3) ^ d(6)                              # 0x79: bits 6, 5, 4, 3, 0 of r
    y = d(0) ^ d(2) ^ d(3) ^ d(5) ^ d(6)                              # 0x5b: bits 6, 4, 3, 1, 0
    coded = np.stack([x, y], axis=1).reshape(-1)
    pat = puncture(po, cr)
    keep = np.tile(pat, -(-len(coded) // len(pat)))[:len(coded)] != 0
    return coded[keep]


def make_stream(po, cr, total_out, seed):
    """message of total_out + ntraceback bytes and its noise-free soft values (> 0: coded bit 0), padded with one erasure to an even count (n_soft is the
    decoder's input byte count times m = 2; the decoder reads no value behind the stream's last step)"""
    rng = np.random.RandomState(seed)
    msg = rng.randint(0, 256, total_out + NTB[cr]).astype(np.uint8)
    soft = (8 - 16 * encode(po, cr, msg).astype(np.int32)).astype(np.int8)
    if len(soft) & 1:
        soft = np.concatenate([soft, np.zeros(1, np.int8)])
    return msg, soft


def add_noise(soft, sigma, seed):
    rng = np.random.RandomState(seed)
    return np.clip(np.rint(soft + sigma * rng.randn(len(soft))), -31, 31).astype(np.int8)


def model(po, cr, soft, n_soft, total_steps, B, nsteps):
    L = po.lib()
    L.o_soft_viterbi.restype = C.c_longlong
    L.o_soft_viterbi.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    c = po.cfg(QPSK, cr, T2k)
    out = np.full(max(total_steps // 8, 0) + 64, 0xA5, np.uint8)
    soft = np.ascontiguousarray(soft, dtype=np.int8)
    n = L.o_soft_viterbi(C.byref(c), _p(soft), n_soft, total_steps, B, nsteps, _p(out))
    return int(n), out


def gpu(g, cr, soft, n_soft, total_steps, B, nsteps, grid, cap=None):
    cap = max(total_steps // 8, 0) + 64 if cap is None else cap
    out = np.zeros(cap, np.uint8)
    soft = np.ascontiguousarray(soft, dtype=np.int8)
    r = g.lib().dvbt_debug_soft_viterbi(QPSK, cr, _p(soft), n_soft, total_steps, B, nsteps, grid, _p(out), cap)
    assert r == 0, (r, g.lib().dvbt_last_error())
    return out


def check(po, g, cr, soft, total_steps, B, grid=1, n_soft=None, what=""):
    """kernel == model on [0, total_out), 0xA5 behind; returns the model's bytes"""
    n_soft = len(soft) if n_soft is None else n_soft
    nsteps = nsteps_for(B, cr)
    n, ref = model(po, cr, soft, n_soft, total_steps, B, nsteps)
    assert n == max(total_steps // 8 - NTB[cr], 0)
    out = gpu(g, cr, soft, n_soft, total_steps, B, nsteps, grid)
    bad = np.flatnonzero(out[:n] != ref[:n])
    assert len(bad) == 0, (what, RATE_IDS[cr], B, nsteps, grid, len(bad), bad[:8], bad[-1])
    assert (ref[n:] == 0xA5).all()
    untouched = np.flatnonzero(out[n:] != 0xA5)
    assert len(untouched) == 0, (what, RATE_IDS[cr], B, grid, n + untouched[:8])
    return ref[:n]


def ber(a, b):
    return float(np.unpackbits(a ^ b).mean())


def _noisy(po, cr, B, seed, total_out=None):
    total_out = total_for(B) if total_out is None else total_out
    msg, clean = make_stream(po, cr, total_out, seed)
    return msg, add_noise(clean, SIGMA[cr], seed + 1), 8 * len(msg)


@pytest.mark.parametrize("cr", [0, 1, 2, 3, 4], ids=[RATE_IDS[i] for i in range(5)])
def test_every_chunk_size(po, g, cr):
    """twelve chunk sizes x one workgroup that makes three passes over its tasks, on a noisy stream"""
    for B in SIZES:
        msg, soft, steps = _noisy(po, cr, B, 100 + 7 * cr + B)
        ref = check(po, g, cr, soft, steps, B, what="sizes")
        e = ber(ref, msg[:len(ref)])
        print(f"rate {RATE_IDS[cr]} B {B} S {-(-(B + 2) // 48) * 6} nsteps {nsteps_for(B, cr)} bytes {len(ref)} model BER {e:.5f}")
        assert 0 < e < 0.12, (RATE_IDS[cr], B, e)


def test_grid_does_not_change_a_byte(po, g):
    """the same stream through 1, 2, 3 workgroups and through the launch's own choice (s4_grid's formula at this B): a decoder's bytes depend on nothing its
    wavefront's slot, LDS rows or best-cell table kept from the task before"""
    cr, B = 4, 143
    total_out = 4 * B * 22 + B // 3 + 1                               # 23 tasks: the launch's own grid is 6
    msg, soft, steps = _noisy(po, cr, B, 31, total_out)
    own = -(-(-(-total_out // (4 * B))) // 4)
    assert own == 6
    for grid in (1, 2, 3, own):
        ref = check(po, g, cr, soft, steps, B, grid=grid, what="grid")
    assert 0 < ber(ref, msg[:len(ref)]) < 0.12


def _bursts(soft, rng):
    s = soft.copy()
    pos = 0
    while True:
        pos += rng.randint(300, 3000)
        n = rng.randint(200, 2001)
        if pos + n >= len(s):
            return s
        s[pos:pos + n] = 0
        pos += n


@pytest.mark.parametrize("cr", [0, 3, 4], ids=[RATE_IDS[i] for i in (0, 3, 4)])
def test_input_classes(po, g, cr):
    for B in (64, 143, 268):
        rng = np.random.RandomState(1000 * cr + B)
        total_out = total_for(B)
        msg, clean = make_stream(po, cr, total_out, 500 + 11 * cr + B)
        steps, n = 8 * len(msg), len(clean)
        ref = check(po, g, cr, clean, steps, B, what="noise-free")
        assert (ref == msg[:len(ref)]).all()                          # the encoder of this file and the model agree on what the code is
        noisy = add_noise(clean, SIGMA[cr], 600 + B)
        ref = check(po, g, cr, noisy, steps, B, what="gaussian")
        assert 0 < ber(ref, msg[:len(ref)]) < 0.12, (RATE_IDS[cr], B)
        # every compare a tie: the tie rule of the add-compare-select and the smallest-physical-cell rule of the best cells decide every byte
        check(po, g, cr, np.zeros(n, np.int8), steps, B, what="all zero")
        # saturated values, random signs: the largest spread of the 16-bit metrics
        check(po, g, cr, (31 * (1 - 2 * rng.randint(0, 2, n))).astype(np.int8), steps, B, what="random +-31")
        # the all-zero codeword at full confidence: the fastest growth of the best metric between two renormalisations
        ref = check(po, g, cr, np.full(n, 31, np.int8), steps, B, what="all +31")
        assert (ref == 0).all()
        check(po, g, cr, _bursts(clean, rng), steps, B, what="erasure bursts")
        check(po, g, cr, _bursts(noisy, rng), steps, B, what="erasure bursts on noise")
        # the input ends at two thirds of what the steps ask for: erasures from there on
        check(po, g, cr, noisy, steps, B, n_soft=(2 * n // 3) & ~1, what="n_soft at two thirds")


@pytest.mark.parametrize("cr", [0, 4], ids=["1/2", "7/8"])
def test_short_streams(po, g, cr):
    B = 64
    for total_out in (1, 63, 64, 65, 4 * B - 1, 4 * B, 4 * B + 1):
        msg, soft, steps = _noisy(po, cr, B, 40 + total_out, total_out)
        for grid in (1, 2):
            ref = check(po, g, cr, soft, steps, B, grid=grid, what=f"total_out {total_out}")
            assert len(ref) == total_out
    # total_steps / 8 - ntraceback <= 0: nothing may be written
    soft = add_noise(np.full(4096, 8, np.int8), 4.0, 3)
    for steps in (8 * NTB[cr], 8 * NTB[cr] - 8, 8 * NTB[cr] + 7, 8, 0):
        out = gpu(g, cr, soft, len(soft), steps, B, nsteps_for(B, cr), 1, cap=256)
        assert (out == 0xA5).all(), steps


def test_arguments_no_plan_produces_are_refused(g):
    """each is refused with DVBT_ERR_INVALID before anything is allocated or launched (out_host stays as the caller left it)"""
    cr, B = 1, 100
    ns, steps = nsteps_for(B, cr), 8 * 400
    soft = np.full(steps * 3 // 2, 8, np.int8)                        # the all-zero codeword
    out = np.full(1024, 0x3C, np.uint8)
    L = g.lib()

    def call(B=B, ns=ns, grid=1, cap=len(out), steps=steps, n_soft=len(soft), const=QPSK, rate=cr):
        r = L.dvbt_debug_soft_viterbi(const, rate, _p(soft), n_soft, steps, B, ns, grid, _p(out), cap)
        assert (out == 0x3C).all() or r == 0
        return r
    assert call() == 0 and (out[:400 - NTB[cr]] == 0).all() and (out[400 - NTB[cr]:] == 0xA5).all()
    out[:] = 0x3C
    assert ns == 1200 and ns % 48 == 0
    bad = [dict(B=63), dict(B=305), dict(B=0), dict(B=-64),
           dict(ns=ns + 8), dict(ns=ns + 24), dict(ns=ns - 1),                       # not a multiple of 48
           dict(ns=S4_MAXSTEPS + 48), dict(ns=48 * 1000),                            # above S4_MAXSTEPS
           dict(ns=ns - 48), dict(ns=48), dict(ns=0), dict(ns=-48),                  # below 256 + 8 B + max(8 ntb, 128)
           dict(B=304, ns=nsteps_for(304, cr) - 48), dict(rate=4, ns=nsteps_for(B, 4) - 48),
           dict(grid=0), dict(grid=-1), dict(grid=2049), dict(grid=1 << 20),
           dict(cap=steps // 8 - 1), dict(cap=0),
           dict(n_soft=-2), dict(n_soft=len(soft) - 1), dict(steps=-8),              # (n_soft counts whole input bytes of m = 2 values)
           dict(const=3), dict(rate=5)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(rate=4, ns=nsteps_for(B, 4)) == 0                                    # (the step count the refused rate 7/8 call was one block short of)
    assert L.dvbt_debug_soft_viterbi(QPSK, cr, None, 0, steps, B, ns, 1, _p(out), len(out)) == -1


# ---------------------------------------------------------------- the demapper
def _axis_boundaries(c):
    n = 1 << (c.m // 2)
    s = np.float32(2.0) * np.float32(c.norm)
    return np.array([np.float32(k) * s for k in range(-(n // 2 - 1), n // 2)], np.float32), float(s)


def _demap_inputs(po, c, rng):
    P = c.payload
    pts = np.zeros(c.csize, np.complex64)
    po.lib().o_constellation(C.byref(c), C.c_float(1.0), _p(pts))
    bnd, s = _axis_boundaries(c)
    eq = np.zeros((4, P), np.complex64)
    for sy in range(4):
        kind = rng.randint(0, 6, P)
        e = (pts[rng.randint(0, c.csize, P)] + 0.2 * s * (rng.randn(P) + 1j * rng.randn(P))).astype(np.complex64)   # kinds 0..2: points plus noise
        re, im = e.real.copy(), e.imag.copy()
        b = bnd[rng.randint(0, len(bnd), P)]
        side = rng.randint(0, 3, P)                                   # exactly on a decision boundary / the nearest float below / above it
        b = np.where(side == 0, b, np.nextafter(b, np.where(side == 1, -np.inf, np.inf).astype(np.float32)))
        ax = rng.randint(0, 3, P)                                     # of the I axis, the Q axis, both
        on = (kind == 3) | (kind == 4)
        re = np.where(on & (ax != 1), b, re)
        im = np.where(on & (ax != 0), np.roll(b, 1), im)
        far = kind == 5                                               # far outside the constellation, up to 100 x norm
        mag = (10 ** rng.uniform(0, 2, P) * c.norm).astype(np.float32)
        ph = rng.uniform(0, 2 * np.pi, P)
        re = np.where(far, mag * np.cos(ph), re)
        im = np.where(far, mag * np.sin(ph), im)
        eq[sy].real, eq[sy].imag = re.astype(np.float32), im.astype(np.float32)
    csi = np.zeros((4, P), np.float32)
    csi[0] = 10 ** rng.uniform(-4, 4, P)                              # eight decades
    csi[1] = 0.37                                                     # constant: every weight is 1
    csi[2] = 2.5e-3; csi[2, rng.randint(0, P)] = 2.5                  # one carrier 1000 x the others: its weight is capped at 4
    csi[3] = 0.0                                                      # no channel power at all: every soft value 0
    parity = np.array([0, 1, 0, 1], np.int32)
    assert np.isfinite(eq.view(np.float32)).all() and np.isfinite(csi).all()
    return pts, eq, csi, parity


@pytest.mark.parametrize("mode", [0, 1], ids=["2k", "8k"])
@pytest.mark.parametrize("const", [0, 1, 2], ids=["QPSK", "QAM16", "QAM64"])
def test_demapper(po, g, const, mode):
    c = po.cfg(const, po.C1_2, mode)
    P, m, pa = c.payload, c.m, c.m // 2
    rng = np.random.RandomState(70 + 3 * const + mode)
    pts, eq, csi, parity = _demap_inputs(po, c, rng)
    out = np.full((4, P * m), 99, np.int8)
    r = g.lib().dvbt_debug_soft_demap(const, mode, _p(eq), _p(csi), _p(parity), 4, _p(out))
    assert r == 0, g.lib().dvbt_last_error()
    # (a) the model, identical
    L = po.lib()
    L.o_soft_demap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    ref = np.zeros((4, P * m), np.int8)
    L.o_soft_demap(C.byref(c), _p(eq), _p(csi), _p(parity), 4, _p(ref))
    bad = np.argwhere(out != ref)
    assert len(bad) == 0, (len(bad), bad[:5])
    assert (out[3] == 0).all() and np.abs(out).max() == 31
    # (b) the formula in float64: levels of the oracle's constellation, weight min(csi / mean, 4), unit 8 per squared step, per carrier and label bit ...
    lev = np.zeros((2, 1 << pa))
    for a in range(2):
        for u in range(1 << pa):
            label = 0
            for jj in range(pa):
                label |= ((u >> (pa - 1 - jj)) & 1) << (m - 1 - (2 * jj + a))
            lev[a, u] = pts[label].imag if a else pts[label].real
    step = 2.0 * float(c.norm)
    v64 = np.zeros((4, P, m))
    for sy in range(4):
        mean = csi[sy].astype(np.float64).sum() / P
        w = np.minimum(csi[sy].astype(np.float64) / mean, 4.0) if mean > 0 else np.zeros(P)
        for a in range(2):
            z = (eq[sy].imag if a else eq[sy].real).astype(np.float64)
            d = (z[:, None] - lev[a][None, :]) ** 2
            for jj in range(pa):
                one = ((np.arange(1 << pa) >> (pa - 1 - jj)) & 1) == 1
                v64[sy, :, 2 * jj + a] = (d[:, one].min(axis=1) - d[:, ~one].min(axis=1)) / step ** 2 * w * 8.0
    # ... moved to the soft values' places by the oracle's hard chain applied to POSITIONS: position byte planes go through o_sym_interleave (direction 0) and
    # the per-bit source through o_bit_deinterleave of one-hot labels
    src_c, src_e = _placement(po, c)
    bnd, s = _axis_boundaries(c)
    worst = (0.0, None)
    for sy in range(4):
        got = out[sy].astype(np.float64)
        want = np.clip(v64[sy][src_c[parity[sy]], src_e[parity[sy]]], -31, 31)
        err = np.abs(got - want)
        k = int(err.argmax())
        if err[k] > worst[0]:
            worst = (float(err[k]), (sy, k, int(out[sy, k]), float(want[k])))
    print(f"demapper const {const} mode {mode}: largest |gpu - float64| {worst[0]:.6f} at {worst[1]}")
    assert worst[0] <= 0.5 + 1e-3, worst
    # (c) placement, independently of the model's table: carriers at least a quarter step from every boundary on both axes and with a weight of at least 1/4
    # have |value| >= 16 * (1/4) * (1/4) = 1 before rounding, so the sign of every one of their soft values is the hard decision's bit; the hard decisions go
    # through the oracle's demap -> symbol de-interleaver -> bit de-interleaver, and so does the mask of those carriers
    H = np.zeros(P, np.int32)
    po.lib().o_sym_H(C.byref(c), _p(H))
    for sy in range(3):
        mean = csi[sy].astype(np.float64).sum() / P
        w = csi[sy].astype(np.float64) / mean
        dist = np.minimum(np.abs(eq[sy].real.astype(np.float64)[:, None] - bnd[None, :]).min(axis=1),
                          np.abs(eq[sy].imag.astype(np.float64)[:, None] - bnd[None, :]).min(axis=1))
        ok = (dist >= 0.25 * s * (1 + 1e-6)) & (w >= 0.25 * (1 + 1e-6))
        labels = np.zeros(P, np.uint8)
        po.lib().o_demap(C.byref(c), _p(pts), _p(np.ascontiguousarray(eq[sy])), _p(labels), C.c_size_t(P))
        hard = _hard_chain(po, c, H, labels, int(parity[sy]))
        mask = _hard_chain(po, c, H, np.where(ok, c.csize - 1, 0).astype(np.uint8), int(parity[sy])) != 0
        assert mask.sum() == ok.sum() * m and ok.sum() > (P // 4 if sy else 20), (sy, int(ok.sum()))
        bits = (out[sy] < 0).astype(np.uint8)
        wrong = np.flatnonzero(mask & (bits != hard))
        assert len(wrong) == 0, (sy, len(wrong), wrong[:8])


def _hard_chain(po, c, H, labels, par):
    """label bytes of one symbol -> symbol de-interleaver -> bit de-interleaver -> the P m bits in the decoder's input order (MSB of a word first)"""
    P = c.payload
    a, b = np.zeros(P, np.uint8), np.zeros(P, np.uint8)
    po.lib().o_sym_interleave(C.byref(c), _p(H), _p(np.ascontiguousarray(labels)), _p(a), par, 0)
    po.lib().o_bit_deinterleave(C.byref(c), _p(a), _p(b), C.c_size_t(P))
    return ((b[:, None] >> np.arange(c.m - 1, -1, -1)[None, :]) & 1).astype(np.uint8).reshape(-1)


def _placement(po, c):
    """for either parity: (carrier, label bit) whose soft value lands at place x, read off the oracle's hard chain: the carrier number in byte planes of labels
    (m bits a plane), the label bit from one-hot labels"""
    P, m = c.payload, c.m
    H = np.zeros(P, np.int32)
    po.lib().o_sym_H(C.byref(c), _p(H))
    src_c, src_e = [], []
    for par in (0, 1):
        car = np.zeros(P * m, np.int64)
        q = np.arange(P)
        # a plane carries ONE bit of the carrier number in all m label bits: behind the chain every place knows that bit of its carrier
        for bit in range(13):
            plane = np.where((q >> bit) & 1, c.csize - 1, 0).astype(np.uint8)
            car |= _hard_chain(po, c, H, plane, par).astype(np.int64) << bit
        e = np.zeros(P * m, np.int64)
        for j in range(m):                                            # label bit j, MSB first, set in every carrier
            got = _hard_chain(po, c, H, np.full(P, 1 << (m - 1 - j), np.uint8), par)
            assert ((e == 0) | (got == 0)).all()
            e = np.where(got != 0, j, e)
        src_c.append(car); src_e.append(e)
        assert (np.bincount(car * m + e, minlength=P * m) == 1).all()  # a permutation of (carrier, bit)
    return src_c, src_e
