"""Pin the oracle's Viterbi restatement bit-for-bit against the REFERENCE's own kernels.

oracle/_ref/libdviterbi_ref.so is lib/d_viterbi.c + lib/d_tab.c + lib/d_metrics.c compiled
unmodified (oracle/Makefile target `ref`).  Both are driven in the calling pattern of
viterbi_decoder_impl::general_work (lib/viterbi_decoder_impl.cc:261-292): butterfly2 every 4
depunctured symbols, get_output when in_count % 16 == 8.

Where oracle/_ref is not built, the oracle is compared with what those kernels produced on the same
inputs, recorded in tests/golden/viterbi_kernels_ref.npz / .json (tests/golden/make_golden.py
--ref-kernels); where it is built, the recordings are checked against the kernels as well.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viterbi_kernels_ref")


def _golden():
    return np.load(GOLDEN + ".npz"), json.load(open(GOLDEN + ".json"))


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _aligned(n):
    raw = np.zeros(n + 64, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n]


def _run_ref(ref, syms, ntb):
    m0, m1, p0, p1 = (_aligned(64) for _ in range(4))
    ref.d_viterbi_chunks_init_sse2(m0.ctypes.data_as(C.c_void_p), p0.ctypes.data_as(C.c_void_p))
    out = []
    ch = C.c_ubyte()
    ref.d_viterbi_get_output_sse2.restype = C.c_ubyte
    for ic in range(0, len(syms), 4):
        s = syms[ic:ic + 4]
        ref.d_viterbi_butterfly2_sse2(s.ctypes.data_as(C.c_void_p), m0.ctypes.data_as(C.c_void_p),
                                      m1.ctypes.data_as(C.c_void_p), p0.ctypes.data_as(C.c_void_p),
                                      p1.ctypes.data_as(C.c_void_p))
        if ic > 0 and ic % 16 == 8:
            ref.d_viterbi_get_output_sse2(m0.ctypes.data_as(C.c_void_p), p0.ctypes.data_as(C.c_void_p),
                                          ntb, C.byref(ch))
            out.append((ch.value, bytes(m0)))
    return out


def _run_oracle(po, syms, ntb):
    L = po.lib()
    v = po.VitCore()
    L.o_vit_core_init(C.byref(v), ntb)
    out = []
    for ic in range(0, len(syms), 4):
        s = syms[ic:ic + 4]
        L.o_vit_butterfly2(C.byref(v), s.ctypes.data_as(C.c_void_p))
        if ic > 0 and ic % 16 == 8:
            ch = L.o_vit_get_output(C.byref(v))
            out.append((ch, bytes(v.metric)))
    return out


def _encode(ref, data, key):
    """the reference's encoder (d_encode) on data: run where oracle/_ref is built (and checked against the recording), else the recording"""
    want = np.unpackbits(np.load(GOLDEN + ".npz")["enc_" + key])[:len(data) * 16]
    if ref is None:
        return want
    sym = np.zeros(len(data) * 16, np.uint8)
    ref.d_encode(sym.ctypes.data_as(C.c_void_p), data.ctypes.data_as(C.c_void_p), len(data), 0)
    assert (sym == want).all(), "recorded encoder output differs from the reference kernels'"
    return sym


def _kernels_case(ref, ntb, ber):
    """the input of test_oracle_viterbi_equals_reference_kernels and, where oracle/_ref is built, the reference kernels' output on it"""
    rng = np.random.RandomState(100 + ntb)
    nbytes = 1400
    data = rng.randint(0, 256, nbytes).astype(np.uint8)
    sym = _encode(ref, data, "ntb%d" % ntb)
    flips = rng.rand(len(sym)) < ber
    sym = (sym ^ flips).astype(np.uint8)
    p = np.array(PUNCT[ntb], np.uint8)
    mask = np.tile(p, len(sym) // len(p) + 1)[:len(sym)]
    sym[mask == 0] = 2                      # erasures exactly as the block's depuncturer inserts them
    n = (len(sym) // 16) * 16
    return data, sym[:n], (_run_ref(ref, sym[:n], ntb) if ref is not None else None)


def _megabyte_case(po, const, cr, ber):
    """~1 MB of decoder input: the oracle chain's clean decoder input, repeated, with independent bit errors"""
    c = po.cfg(const, cr, po.T2k)
    blk_in = 768 * c.n // c.m
    nblocks = 1000000 // blk_in
    # a coded stream: random payload through the reference's own encoder + puncturing would need the kernels' d_encode; the decoder's behaviour under comparison does not
    # depend on the input being a codeword, so: the oracle chain's clean decoder input, repeated, with independent bit errors
    ibits = c.payload * c.m * c.k // c.n
    iq = po.tx(c, po.make_ts((272 * ibits * 2) // (204 * 8), 5), lead_in=500, tail=3 * c.N)
    vin = po.rx(c, iq, want=("bitdeint",))["bitdeint"].reshape(-1)
    vin = np.tile(vin, nblocks * blk_in // len(vin) + 1)[:nblocks * blk_in].copy()
    rng = np.random.RandomState(17)
    for b in range(c.m):
        vin ^= (rng.rand(len(vin)) < ber).astype(np.uint8) << b
    return c, vin


def _ref_decode_n(po, c, vin):
    """the block loop around the REFERENCE's own kernels (oracle/o_refbench.c::o_ref_viterbi_decode_n), None where oracle/_ref is not built"""
    if not os.path.exists(po._REF):
        return None
    L = po.lib()
    L.o_ref_viterbi_decode_n.restype = C.c_size_t
    L.o_ref_viterbi_decode_n.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    r = np.zeros(len(vin) * c.m * c.k // (8 * c.n) + 64, np.uint8)
    nr = L.o_ref_viterbi_decode_n(po._REF.encode(), C.byref(c), vin.ctypes.data, len(vin), r.ctypes.data)
    assert nr != 2 ** 64 - 1, "reference kernels could not be loaded"
    return r[:nr]


MEGABYTE_CASES = [(2, 4, 0.0), (2, 4, 0.02), (2, 4, 0.06), (2, 4, 0.5), (0, 4, 0.06), (1, 0, 0.5), (2, 2, 0.08), (2, 3, 0.5)]


PUNCT = {5: [1, 1], 9: [1, 1, 0, 1], 10: [1, 1, 0, 1, 1, 0], 15: [1, 1, 0, 1, 1, 0, 0, 1, 1, 0],
         24: [1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0]}


@pytest.mark.parametrize("ntb", [5, 9, 10, 15, 24])
@pytest.mark.parametrize("ber", [0.0, 0.02, 0.08])
def test_oracle_viterbi_equals_reference_kernels(po, ntb, ber):
    ref = po.ref_lib()
    data, sym, a = _kernels_case(ref, ntb, ber)
    n = len(sym)
    key = "ntb%d_ber%g" % (ntb, ber)
    g, meta = _golden()
    if a is not None:                       # the recording is what the kernels produce
        assert [x[0] for x in a] == list(g["dec_" + key]) and _sha(b"".join(x[1] for x in a)) == meta["metrics_sha256"][key]
    b = _run_oracle(po, sym, ntb)
    assert len(b) == n // 16 == len(g["dec_" + key])
    assert [x[0] for x in b] == list(g["dec_" + key])                       # decoded bytes
    assert _sha(b"".join(x[1] for x in b)) == meta["metrics_sha256"][key]    # renormalised metrics after every output
    dec = np.array([x[0] for x in b], np.uint8)
    if ber == 0.0:
        # SURVEY App. F "Viterbi delay": out[i+T] == data[i]
        assert (dec[ntb:] == data[:len(dec) - ntb]).all()


def test_block_decode_matches_stream(po):
    """o_viterbi_decode (block restatement incl. depuncture) == kernels driven by hand."""
    ref = po.ref_lib()
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    rng = np.random.RandomState(5)
    data = rng.randint(0, 256, 672 * 3).astype(np.uint8)
    sym = _encode(ref, data, "block")
    p = np.array(PUNCT[24], np.uint8)
    mask = np.tile(p, len(sym) // 14 + 1)[:len(sym)]
    kept = sym[mask == 1]
    nb = len(kept) // 6
    packed = np.zeros(nb, np.uint8)
    for j in range(6):
        packed |= (kept[j:nb * 6:6] << (5 - j)).astype(np.uint8)
    out = np.zeros(len(data) + 64, np.uint8)
    n = po.lib().o_viterbi_decode(C.byref(c), 768, packed.ctypes.data_as(C.c_void_p), len(packed),
                                  out.ctypes.data_as(C.c_void_p))
    assert n == 672 * 3 - 24
    assert (out[:n] == data[:n]).all()


@pytest.mark.parametrize("const,cr,ber", MEGABYTE_CASES)
def test_oracle_block_decode_equals_reference_kernels_on_megabytes(po, const, cr, ber):
    """The block-level restatement (o_viterbi_decode_n: depuncturer + butterfly / output cadence) against the same loop around the REFERENCE's own kernels, driven
    natively (oracle/o_refbench.c::o_ref_viterbi_decode_n), on ~1 MB of decoder input per case: clean, at the edge of what the code copes with, on collapsed channels and on
    garbage -- the regimes in which the product's chunked decoder is compared with this restatement (tests/test_gpu_warmup.py, tools/hier_warmup.py)."""
    c, vin = _megabyte_case(po, const, cr, ber)
    L = po.lib()
    L.o_viterbi_decode_n.restype = C.c_size_t
    L.o_viterbi_decode_n.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    a = np.zeros(len(vin) * c.m * c.k // (8 * c.n) + 64, np.uint8)
    na = L.o_viterbi_decode_n(C.byref(c), vin.ctypes.data, len(vin), a.ctypes.data)
    want = _golden()[1]["megabyte"]["c%d_r%d_ber%g" % (const, cr, ber)]
    r = _ref_decode_n(po, c, vin)
    if r is not None:                       # the recording is what the kernels produce
        assert len(r) == want["n"] and _sha(r) == want["sha256"]
        assert na == len(r) and (a[:na] == r).all()
    assert na == want["n"] > 100000 and _sha(a[:na]) == want["sha256"]
