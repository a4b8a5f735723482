"""dvbt_rx_quality on the GPU: the two counting kernels alone through their hooks against the model tests/qualref.py (every span edge, every code rate and
constellation, clipped inputs), and the whole measurement behind a decoded segment against the model applied to the GPU's OWN taps -- the noisy cases are not
compared with the oracle's counts, because the GPU's decoder input may differ from the oracle's in a few bits at decision boundaries; the fixture pins the
model (tests/test_quality_model.py), the GPU is pinned to the model here."""
import ctypes as C

import numpy as np
import pytest

import qualcases
import qualref

pytestmark = pytest.mark.gpu

RATE_IDS = {0: "1/2", 1: "2/3", 2: "3/4", 3: "5/6", 4: "7/8"}
N_VIT = (1, 2, 3, 7, 8, 9, 23, 24, 25, 191, 192, 193, 4097)
ERR_INVALID, ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    L = gr_dvbt_amd.lib()
    L.dvbt_debug_quality_channel.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dvbt_debug_quality_post.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dvbt_rx_quality.argtypes = [C.c_void_p, C.POINTER(gr_dvbt_amd.RxQuality)]
    return gr_dvbt_amd


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def hook_channel(g, m, cr, inp, vit):
    a, e = C.c_int64(-1), C.c_int64(-1)
    inp = np.ascontiguousarray(inp, np.uint8)
    vit = np.ascontiguousarray(vit, np.uint8)
    pad_in, pad_vit = np.concatenate([inp, np.zeros(8, np.uint8)]), np.concatenate([vit, np.zeros(8, np.uint8)])      # (never a null pointer for an empty array)
    r = g.lib().dvbt_debug_quality_channel(m // 2 - 1, cr, _p(pad_in), len(inp), _p(pad_vit), len(vit), C.byref(a), C.byref(e))
    assert r == 0, g.lib().dvbt_last_error()
    return a.value, e.value


def hook_post(g, vit, rs, n_words):
    a, e = C.c_int64(-1), C.c_int64(-1)
    vit = np.ascontiguousarray(vit, np.uint8)
    rs = np.ascontiguousarray(rs, np.uint8)
    r = g.lib().dvbt_debug_quality_post(_p(vit), len(vit), _p(rs), n_words, C.byref(a), C.byref(e))
    assert r == 0, g.lib().dvbt_last_error()
    return a.value, e.value


def flip(inp, m, qs):
    out = inp.copy()
    for q in qs:
        out[q // m] ^= 1 << (m - 1 - q % m)
    return out


@pytest.mark.parametrize("m", [2, 4, 6])
@pytest.mark.parametrize("cr", [0, 1, 2, 3, 4], ids=lambda c: RATE_IDS[c])
def test_channel_kernel_counts_what_the_model_counts(g, cr, m):
    rng = np.random.RandomState(7000 + 10 * cr + m)
    for n_vit in N_VIT:
        vit = rng.randint(0, 256, n_vit).astype(np.uint8)
        tail = rng.randint(0, 2, 8 * 24 + 5).astype(np.uint8)                       # the input goes on behind the decoded bytes, as the chain's does
        inp = qualref.puncture_pack(np.concatenate([qualref.info_bits(vit), tail]), cr, m)
        q, _ = qualref.counted_set(n_vit, len(inp), m, cr)
        assert hook_channel(g, m, cr, inp, vit) == (len(q), 0), n_vit
        if n_vit < 2:
            assert len(q) == 0
            continue
        # up to 50 flipped bits: the first and the last counted bit, others anywhere in the counted set, and one in front of it (step < 8) that must not count
        K = min(50, len(q))
        inside = np.unique(np.concatenate([[q[0], q[-1]], rng.choice(q, K - 2, replace=False)])) if K > 2 else np.unique([q[0], q[-1]])
        assert q[0] > 0
        bad = flip(inp, m, list(inside) + [int(rng.randint(0, q[0]))])
        want = qualref.channel_errors(bad, vit, m, cr)
        assert want == (len(q), len(inside))
        assert hook_channel(g, m, cr, bad, vit) == want, n_vit
    # the clip: an input that ends with the decoded bytes' own last whole byte, and one byte short of that
    n_vit = 193
    vit = rng.randint(0, 256, n_vit).astype(np.uint8)
    inp = qualref.puncture_pack(qualref.info_bits(vit), cr, m)
    for cut in (0, 1):
        short = inp[:len(inp) - cut]
        q, _ = qualref.counted_set(n_vit, len(short), m, cr)
        full, _ = qualref.counted_set(n_vit, len(inp) + 64, m, cr)
        assert len(q) < len(full) or (cut == 0 and len(q) == len(full))
        bad = flip(short, m, [q[0], q[-1], q[len(q) // 2]])
        want = qualref.channel_errors(bad, vit, m, cr)
        assert want == (len(q), 3)
        assert hook_channel(g, m, cr, bad, vit) == want
    short = inp[:len(inp) - 1]
    assert len(qualref.counted_set(n_vit, len(short), m, cr)[0]) < len(qualref.counted_set(n_vit, len(inp) + 64, m, cr)[0])


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("n_words", [1, 11, 12, 13, 100])
def test_post_kernel_counts_the_flipped_bits(g, n_words, extra):
    rng = np.random.RandomState(8000 + n_words + extra)
    vit = rng.randint(0, 256, 204 * n_words + extra).astype(np.uint8)
    rs = qualref.deint_from_viterbi(vit, n_words).reshape(n_words, 204)[:, :188].copy()
    assert hook_post(g, vit, rs, n_words) == (1504 * n_words, 0)
    flips = {(0, 0, 0x01), (0, 187, 0x80), (n_words - 1, 0, 0x80), (n_words - 1, 187, 0x01)}
    for _ in range(40):
        flips.add((int(rng.randint(n_words)), int(rng.randint(188)), 1 << int(rng.randint(8))))
    bad = rs.copy()
    for w, p, bit in flips:
        bad[w, p] ^= bit
    nbits = int(np.unpackbits(bad ^ rs).sum())
    assert nbits >= 4
    assert qualref.post_errors(qualref.deint_from_viterbi(vit, n_words), bad) == (1504 * n_words, nbits)
    assert hook_post(g, vit, bad, n_words) == (1504 * n_words, nbits)


_iq = {}


def case_iq(po, name):
    if name not in _iq:
        _iq[name] = qualcases.make_iq(po, qualcases.case(name))
    return _iq[name]


def raw(q):
    return C.string_at(C.addressof(q), C.sizeof(q))


@pytest.mark.parametrize("name", qualcases.ONE_PERIOD)
def test_chain_one_period(g, po, name):
    c = qualcases.case(name)
    cfg, iq = case_iq(po, name)
    kw = dict(max_samples=len(iq), snr_db=qualcases.rx_snr(c))
    rx = g.Rx(c[1], c[2], c[3], quality=True, **kw)
    rep = rx.run(iq)
    q = rx.quality()
    q2 = rx.quality()
    assert raw(q) == raw(q2)                                        # bit for bit, the float sums included
    assert rep.n_lock_periods == 1 and q.flags == 0 and q.n_lock_periods == 1
    assert (q.rs_fail_words, q.rs_corrected_symbols) == (rep.rs_fail_words, rep.rs_corrected_symbols)
    eq, bitdeint, vit, rs, ts = (rx.tap(t) for t in (g.TAP_EQ, g.TAP_BITDEINT, g.TAP_VITERBI, g.TAP_RS, g.TAP_TS))
    rx.close()
    # a second handle with the debug taps for DEINT, a third, plain one: same stream, same bytes, same counts
    rt = g.Rx(c[1], c[2], c[3], taps=True, **kw)
    rt.run(iq)
    deint = rt.tap(g.TAP_DEINT)
    assert np.array_equal(rt.tap(g.TAP_RS), rs) and np.array_equal(rt.tap(g.TAP_VITERBI), vit)
    rt.close()
    plain = g.Rx(c[1], c[2], c[3], **kw)
    plain.run(iq)
    ts_plain = plain.tap(g.TAP_TS)
    qp = plain.quality()
    assert np.array_equal(plain.tap(g.TAP_TS), ts_plain) and np.array_equal(ts_plain, ts) and len(ts) > 0      # the measurement changed nothing
    plain.close()

    words = len(rs) // 188
    assert np.array_equal(qualref.deint_from_viterbi(vit, words), deint)
    ch = qualref.channel_errors(bitdeint, vit, cfg.m, c[2])
    post = qualref.post_errors(deint, rs)
    n, sig, err = qualref.mer(eq, cfg.m, cfg.norm)
    print(name, "GPU", q.channel_bit_errors, "/", q.channel_bits, q.post_bit_errors, "/", q.post_bits, "MER", q.mer_db, "model", ch, post, qualref.mer_db(sig, err),
          "signal", q.mer_signal, sig, "error", q.mer_error, err)
    assert (q.channel_bits, q.channel_bit_errors) == ch and ch[0] > 0
    assert (q.post_bits, q.post_bit_errors) == post and post[0] == 1504 * words > 0
    assert q.mer_carriers == n == rep.n_out_symbols * cfg.payload
    assert abs(q.mer_signal - sig) <= 1e-5 * sig
    if c[5] is None:
        # mer_error is a sum of rounding residues here: only its size is asserted (the EQ tap's contract of 1e-3 * 2 norm per component bounds the MER at 61 dB)
        assert q.channel_bit_errors == 0 and q.post_bit_errors == 0 and q.mer_db >= 55.0
    else:
        assert abs(q.mer_error - err) <= 1e-5 * err
        assert abs(q.mer_db - qualref.mer_db(sig, err)) < 1e-3
        assert q.channel_ber == ch[1] / ch[0] and q.post_viterbi_ber == post[1] / post[0]
    # without dvbt_rx_enable_quality: the same counts, no MER
    assert (qp.channel_bits, qp.channel_bit_errors, qp.post_bits, qp.post_bit_errors) == (q.channel_bits, q.channel_bit_errors, q.post_bits, q.post_bit_errors)
    assert qp.mer_carriers == 0 and qp.flags == 1 and np.isnan(qp.mer_db) and qp.mer_signal == 0.0 and qp.mer_error == 0.0


def test_chain_four_lock_periods(g, po):
    name = "2k_qam16_1_2_4sf_9dB"
    c = qualcases.case(name)
    cfg, iq = case_iq(po, name)
    rx = g.Rx(c[1], c[2], c[3], max_samples=len(iq), snr_db=qualcases.rx_snr(c), taps=True, quality=True)
    rep = rx.run(iq)
    q = rx.quality()
    deint, rs = rx.tap(g.TAP_DEINT), rx.tap(g.TAP_RS)
    rx.close()
    assert rep.n_lock_periods > 1 and q.n_lock_periods == rep.n_lock_periods        # (periods that delivered; the oracle counts four periods with symbols)
    assert q.flags & 2 and q.channel_bits == 0 and q.channel_bit_errors == 0 and q.mer_carriers == 0 and q.mer_signal == 0.0 and q.mer_error == 0.0
    assert np.isnan(q.mer_db) and np.isnan(q.channel_ber)
    post = qualref.post_errors(deint, rs)
    assert (q.post_bits, q.post_bit_errors) == post and post[0] == 1504 * (len(rs) // 188) > 0


def test_enable_order_and_late_enable(g, po):
    """dvbt_rx_enable_quality beside dvbt_rx_enable_taps in either order, and enabled only after the segment ran"""
    name = "2k_qam16_1_2_4sf_12dB"
    c = qualcases.case(name)
    cfg, iq = case_iq(po, name)
    rx = g.Rx(c[1], c[2], c[3], max_samples=len(iq), snr_db=qualcases.rx_snr(c))
    rx.run(iq)
    rx.enable_quality()                                  # the buffer exists now, but no segment has written it
    q = rx.quality()
    assert q.flags == 1 and q.mer_carriers == 0 and q.channel_bits > 0
    rx.run(iq)
    ref = rx.quality()
    assert ref.flags == 0 and ref.mer_carriers > 0
    L = g.lib()
    assert L.dvbt_rx_enable_taps(rx.h, 1) == 0           # the taps take the buffer over ...
    rx.enable_quality(False)                             # ... and keep it
    rx.run(iq)
    assert raw(rx.quality()) == raw(ref) and rx.tap(g.TAP_EQ).size == ref.mer_carriers
    rx.enable_quality(True)
    assert L.dvbt_rx_enable_taps(rx.h, 0) == 0           # dvbt_rx_enable_taps(0) frees what it always freed
    rx.run(iq)
    q = rx.quality()
    assert q.flags == 1 and q.mer_carriers == 0 and (q.channel_bits, q.channel_bit_errors, q.post_bit_errors) == (ref.channel_bits, ref.channel_bit_errors, ref.post_bit_errors)
    rx.enable_quality(True)
    rx.run(iq)
    assert raw(rx.quality()) == raw(ref)
    rx.close()


def test_limits(g, po):
    L = g.lib()
    n = 1 << 20
    out = g.RxQuality()

    def code(rx):
        return L.dvbt_rx_quality(rx.h, C.byref(out))
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=n)
    assert code(rx) == ERR_STATE                         # before any segment
    rx.set_cut(272)
    assert code(rx) == ERR_STATE
    rx.close()
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=n, hierarchy=g.ALPHA2)
    assert code(rx) == ERR_INVALID
    rx.close()
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=n, soft_decision=1)
    assert code(rx) == ERR_STATE
    rx.close()
    # a cut set behind a finished segment is refused too
    name = "2k_qam16_1_2_4sf_12dB"
    c = qualcases.case(name)
    cfg, iq = case_iq(po, name)
    rx = g.Rx(c[1], c[2], c[3], max_samples=len(iq), snr_db=qualcases.rx_snr(c))
    rx.run(iq)
    assert code(rx) == 0
    rx.set_cut(272)
    assert code(rx) == ERR_STATE and "cut" in L.dvbt_last_error().decode()
    rx.close()
