"""The cases in which the oracle's stages are compared with the REFERENCE's own blocks (oracle/refblocks.py), shared by
tests/test_oracle_ref_blocks.py (oracle against the running reference, or against its recordings), tests/golden/make_golden.py --ref-blocks (the recordings)
and tests/test_gpu_ref_blocks.py (the GPU entries against the recordings).

Every case is a dict of plain parameters with a seed; make_input(po, case) regenerates its input from them.  run_ref(case, inp) drives the reference block
(run_ref(case, inp, which="hip"): the project's GNU Radio shell of the same name, on a GPU; tests/test_gpu_gr_shells.py replays the recorded calls instead),
run_oracle(po, case, inp) the oracle's stage function in the same calls; both return
    {"out": [uint8 array per output port], "log": [[noutput_items, returned, consumed], ...] per general_work call, "tags": [[port, offset, key, value], ...]}
(the oracle's "log" / "tags" are None where the oracle has no counterpart of the block's scheduling: then only the reference's are recorded).

What is oracle C and what is restated here.  The outputs always come from the oracle's C functions (o_sym_interleave, o_bit_*, o_viterbi_decode_n,
o_conv_*, o_rs_*, o_energy_*, o_inner_code -- the generator's own coder loop --, o_constellation / o_demap, o_demod_work, o_tx_generate's symbols).  The "log"
and "tags" of the 1:1 blocks are mere call counting.  For kinds "vit" and "convdeint" the REACTION TO A TAG -- the partial block or item pair dropped in front
of it, the re-tag, the first call of a period returning ntraceback bytes less -- is restated in this file (run_oracle, _tagged_stream): a test-side model of
the two blocks' scheduling, checked against the reference like the oracle, not oracle code.  The oracle's own C for it is the period layout of o_chain.c
(with o_conv_deint_taken_before_tag, which the "convdeint" cases in calls of one pair also take their input cut from); o_chain.c is run against the chained
reference blocks by the kind "chain" cases, the lock-lost one for the tag reactions.

TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C
import hashlib

import numpy as np

from . import refblocks as rb

_refblocks = rb

P2K, P8K = 1512, 6048
RS_ARGS = [2, 8, 0x11d, 255, 239, 8, 51, 8]
CONST_NAME = {0: "qpsk", 1: "qam16", 2: "qam64"}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _log_1to1(nitems, calls, per_call_in=1):
    """calls of a block that consumes per_call_in items per output item and returns what it was asked for"""
    log, pos, ci = [], 0, 0
    while True:
        n = calls[min(ci, len(calls) - 1)]
        if pos + n * per_call_in > nitems:
            return log
        log.append([n, n, n * per_call_in])
        pos += n * per_call_in
        ci += 1


# ------------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------------
def _cases():
    cs = {}

    def add(name, **kw):
        assert name not in cs
        kw["name"] = name
        cs[name] = kw

    # symbol (de)interleaver: even and odd indices, a repeated index (2, 2), skipped ones (3 -> 5, 6 -> 67), the frame wrap (67 -> 0); calls of 1 and 3 items
    for mode in (0, 1):
        for direction in (0, 1):
            add("sym_%s_dir%d" % ("8k" if mode else "2k", direction), kind="sym", mode=mode, direction=direction,
                indices=[0, 1, 2, 2, 3, 5, 6, 67, 0, 1, 1, 4], calls=[1, 3], seed=11 + mode * 2 + direction)
    # bit de-interleaver: every constellation, NH and the three hierarchies of 16- and 64-QAM
    for const in (0, 1, 2):
        for hier in ((0,) if const == 0 else (0, 1, 2, 3)):
            add("bitdeint_%s_h%d" % (CONST_NAME[const], hier), kind="bitdeint", const=const, hier=hier, calls=[1, 3], seed=30 + const * 4 + hier)
        add("bitint_%s" % CONST_NAME[const], kind="bitint", const=const, calls=[1, 3], seed=50 + const)
    # the viterbi_decoder block: rates x constellations, clean and 2 % bit errors; tags: only at 0 / a second one at a block boundary / one inside a block
    for const in (0, 1, 2):
        for rate in range(5):
            for ber in (0.0, 0.02):
                add("vit_%s_r%d_ber%g" % (CONST_NAME[const], rate, ber), kind="vit", const=const, rate=rate, ber=ber, nblocks=5, calls=[1, 2],
                    tag_blocks=[0.0], seed=100 + const * 10 + rate)
    add("vit_qam16_r1_tag_boundary", kind="vit", const=1, rate=1, ber=0.02, nblocks=8, calls=[1, 2], tag_blocks=[0.0, 3.0], seed=131)
    add("vit_qam16_r1_tag_boundary_inside_call", kind="vit", const=1, rate=1, ber=0.02, nblocks=8, calls=[1, 2], tag_blocks=[0.0, 2.0], seed=134)
    add("vit_qam64_r2_tag_inside", kind="vit", const=2, rate=2, ber=0.02, nblocks=8, calls=[2, 1], tag_blocks=[0.0, 3.4], seed=132)
    add("vit_qpsk_r4_tag_inside_first_call", kind="vit", const=0, rate=4, ber=0.0, nblocks=7, calls=[1], tag_blocks=[0.25, 4.5], seed=133)
    # Forney byte (de)interleaver: 24 .. 60 RS words, the tag at 0 and at a later byte, pairs of items
    for words in (24, 40, 60):
        add("convint_%dw" % words, kind="convint", words=words, calls=[1, 2], seed=200 + words)
        add("convdeint_%dw_tag0" % words, kind="convdeint", words=words, calls=[2], tags=[0], seed=210 + words)
    add("convdeint_60w_tag_later", kind="convdeint", words=60, calls=[2], tags=[0, 3264 + 700], seed=221)
    add("convdeint_60w_tag_later_only", kind="convdeint", words=60, calls=[2, 4], tags=[1000], seed=222)
    add("convdeint_60w_tag_behind_a_pair", kind="convdeint", words=60, calls=[2], tags=[2 * 3264 + 1], seed=223)
    # Reed-Solomon
    add("rs_enc", kind="rsenc", items=3, calls=[1, 2], seed=300)
    add("rs_dec", kind="rsdec", calls=[1], seed=301)
    # energy dispersal / descramble
    add("disp_aligned", kind="disp", packets=32, lead=0, calls=[1, 2], seed=400)
    add("disp_lead_in", kind="disp", packets=32, lead=77, calls=[1], seed=401)
    for phase in range(8):
        add("descr_phase%d" % phase, kind="descr", phase=phase, groups=12, damage="none", seed=410 + phase)
    add("descr_bad_nsync_at_call_start", kind="descr", phase=3, groups=14, damage="nsync", at=4, seed=420)     # the only place the block looks
    add("descr_bad_nsync_inside_call", kind="descr", phase=3, groups=14, damage="nsync", at=3, seed=422)
    add("descr_sync_lost", kind="descr", phase=5, groups=20, damage="lost", seed=421)
    # inner coder
    for const in (0, 1, 2):
        for rate in range(5):
            add("coder_%s_r%d" % (CONST_NAME[const], rate), kind="coder", const=const, hier=0, rate=rate, calls=[4, 8], seed=500 + const * 5 + rate)
    add("coder_qam64_h2_r2", kind="coder", const=2, hier=2, rate=2, calls=[4], seed=520)
    # mapper / demapper
    for const in (0, 1, 2):
        for hier in ((0,) if const == 0 else (0, 1, 2, 3)):       # NH, alpha 1 / 2 / 4 (hierarchical QPSK does not exist)
            add("demap_%s_h%d" % (CONST_NAME[const], hier), kind="demap", const=const, hier=hier, calls=[1, 2], seed=600 + const * 4 + hier)
            add("map_%s_h%d" % (CONST_NAME[const], hier), kind="map", const=const, hier=hier, calls=[1, 2], seed=620 + const * 4 + hier)
    # demod_reference_signals, one item per call (two visible), fed with the generator's ideal FFT-output symbols; reference_signals fed with their payload
    add("demod_2k_qam16_r0_superframe", kind="demod", const=1, rate=0, mode=0, nsf=3, start=0, nfeed=554, sync=[0], seed=700, keep=[0, 1, 68])
    add("demod_2k_qam64_r4_superframe", kind="demod", const=2, rate=4, mode=0, nsf=3, start=0, nfeed=554, sync=[0], seed=701, keep=[0])
    # (8k 64-QAM: the block takes frame 3 for the superframe's start, demod_reference_signals_impl.cc:73-77; the TPS word of frame 2 is symbols 136 .. 203)
    add("demod_8k_qam64_r4_frame", kind="demod", const=2, rate=4, mode=1, nsf=1, start=130, nfeed=204 - 130 + 68, sync=[0], seed=702)
    add("demod_2k_sync_midstream", kind="demod", const=1, rate=0, mode=0, nsf=3, start=0, nfeed=600, sync=[0, 300], seed=703)
    for i, st in enumerate((1, 17, 67, 68, 69, 135, 136, 203, 271)):
        add("demod_2k_enter_at_%d" % st, kind="demod", const=1, rate=0, mode=0, nsf=3, start=st, nfeed=272 - st + 272 + 6, sync=[0], seed=710 + i)
    add("demod_2k_symbol_dropped", kind="demod", const=1, rate=0, mode=0, nsf=3, start=0, nfeed=560, sync=[0], drop=300, seed=720)
    add("demod_2k_symbol_dropped_before_lock", kind="demod", const=1, rate=0, mode=0, nsf=3, start=0, nfeed=560, sync=[0], drop=240, seed=724)
    add("demod_2k_tps_1_flipped", kind="demod", const=1, rate=0, mode=0, nsf=3, start=0, nfeed=560, sync=[0], tps_flip=[(234, 1)], seed=721)
    add("demod_2k_tps_2_flipped", kind="demod", const=1, rate=0, mode=0, nsf=3, start=0, nfeed=560, sync=[0], tps_flip=[(234, 1), (245, 1)], seed=722)
    add("demod_2k_tps_flipped_after_lock", kind="demod", const=1, rate=0, mode=0, nsf=3, start=0, nfeed=560, sync=[0], tps_flip=[(302, 1), (380, 2)], seed=725)
    add("refsig_2k_qam16", kind="refsig", const=1, rate=0, mode=0, nsym=276, calls=[1, 3], seed=730, keep=[0, 68])
    add("refsig_2k_qam64_cell", kind="refsig", const=2, rate=4, mode=0, nsym=70, calls=[2], seed=731, cell=(1, 0x5a))
    add("refsig_8k_qam64", kind="refsig", const=2, rate=4, mode=1, nsym=70, calls=[1], seed=732)
    # the reference's receive blocks chained, demod_reference_signals to energy_descramble, on the FFT items of a clean loopback: each block in its smallest calls
    # as soon as its input is there (the regime oracle/o_chain.c states), tags handed on by hand; against the oracle chain's taps
    add("chain_2k_qam16_r0", kind="chain", const=1, rate=0, mode=0, seed=800)
    add("chain_2k_qam64_r2", kind="chain", const=2, rate=2, mode=0, seed=801)
    # ... and with the signal gone for three symbols inside the first superframe delivered: the CP lock is lost, the demodulator hunts the next superframe start, the
    # decoder and the byte de-interleaver drop what lies in front of the new tag, the descrambler finds its NSYNC again (two lock periods in o_rx_run)
    add("chain_2k_qam16_r0_lock_lost", kind="chain", const=1, rate=0, mode=0, seed=802, superframes=3.3, gap=(272 + 130, 3))
    return cs


CHAIN_TAPS = ("eq", "demap", "symdeint", "bitdeint", "vit", "deint", "rs", "ts")
CASES = _cases()


# ------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
def _cfg(po, case, mode=0):
    return po.cfg(case.get("const", 1), case.get("rate", 0), case.get("mode", mode), hierarchy=case.get("hier", 0))


def rs_words(po, seed):
    """(204-byte words as sent, the same with symbol errors, list of error positions per word): the all-zero word, clean words, 1 error at the first / last data /
    last parity byte, 8 errors (with the first byte, with the last, spread, all in the parity), 9 errors (beyond the code), 2 and 5 errors"""
    rng = np.random.RandomState(seed)
    plans = [("zero", []), ("clean", []), ("one", [0]), ("one", [187]), ("one", [203]), ("one", [188]),
             ("n", 8, [0]), ("n", 8, [203]), ("n", 8, []), ("par", 8), ("n", 9, [0]), ("n", 9, []), ("n", 2, []), ("n", 5, [187]), ("zero1", [100]), ("clean", [])]
    L = po.lib()
    rs = po.RS()
    L.o_rs_init(C.byref(rs))
    sent = np.zeros((len(plans), 204), np.uint8)
    errpos = []
    for i, p in enumerate(plans):
        w = np.zeros(255, np.uint8)
        if not p[0].startswith("zero"):
            w[51:239] = rng.randint(0, 256, 188)
        L.o_rs_encode(C.byref(rs), _p(w), _p(w[239:]))
        sent[i] = w[51:]
        if p[0] in ("zero", "clean", "one", "zero1"):
            pos = list(p[1])
        elif p[0] == "par":
            pos = list(188 + rng.choice(16, p[1], replace=False))
        else:
            rest = [x for x in rng.permutation(204) if x not in p[2]]
            pos = list(p[2]) + [int(x) for x in rest[:p[1] - len(p[2])]]
        errpos.append(sorted(int(x) for x in pos))
    recv = sent.copy()
    for i, pos in enumerate(errpos):
        for x in pos:
            recv[i, x] ^= rng.randint(1, 256)
    return sent, recv, errpos


def demap_points(po, case):
    """what a demapper can get wrong, as complex64: every constellation point; every midpoint between horizontal, vertical and diagonal neighbours (ties); the
    float just below and just above every decision boundary on lines through the points; the centre gap of alpha 2 / 4 (the origin, the axes); points far
    outside; Gaussian-noisy points"""
    c = _cfg(po, case)
    pts = np.zeros(c.csize, np.complex64)
    po.lib().o_constellation(C.byref(c), C.c_float(1.0), _p(pts))
    re = np.unique(pts.real)
    lv = np.unique(np.concatenate([re, pts.imag])).astype(np.float32)
    mids = ((lv[:-1].astype(np.float64) + lv[1:]) / 2).astype(np.float32)            # decision boundaries of the axis levels
    edge = np.concatenate([mids, np.nextafter(mids, np.float32(-10)), np.nextafter(mids, np.float32(10))]).astype(np.float32)
    out = [pts]
    gx, gy = np.meshgrid(mids, lv)
    out.append((gx + 1j * gy).reshape(-1))                                            # horizontal midpoints
    out.append((gy + 1j * gx).reshape(-1))                                            # vertical midpoints
    gx, gy = np.meshgrid(mids, mids)
    out.append((gx + 1j * gy).reshape(-1))                                            # four-way ties
    gx, gy = np.meshgrid(edge, lv)
    out.append((gx + 1j * gy).reshape(-1))
    out.append((gy + 1j * gx).reshape(-1))
    gx, gy = np.meshgrid(edge, edge)
    out.append((gx + 1j * gy).reshape(-1)[:2000])
    far = np.float32(lv[-1] * 50)
    out.append(np.array([0, far, -far, 1j * far, -1j * far, far + 1j * far, -far - 1j * far, far - 1j * far, 1e-30, -1e-30j, 3e4 + 1j, lv[-1] + 1e-3j * far],
                        np.complex64))
    rng = np.random.RandomState(case["seed"])
    x = np.concatenate([np.asarray(a).astype(np.complex64) for a in out])
    n = 3 * P2K - len(x)                                                               # three items: a call of 1 and a call of 2; the rest is noisy points
    assert n >= 1000
    noisy = pts[rng.randint(0, c.csize, n)] + (0.35 * (lv[1] - lv[0]) * (rng.randn(n) + 1j * rng.randn(n)))
    return np.concatenate([x, noisy.astype(np.complex64)])


def make_input(po, case):
    """the case's input: {"in": [uint8 array per input port], "nitems": items of the block's input size, ...}"""
    k = case["kind"]
    rng = np.random.RandomState(case["seed"])
    L = po.lib()
    if k == "sym":
        P = P8K if case["mode"] else P2K
        x = rng.randint(0, 64, (len(case["indices"]), P)).astype(np.uint8)
        return {"in": [x.reshape(-1)], "nitems": len(x)}
    if k in ("bitdeint", "bitint"):
        v = (2, 4, 6)[case["const"]]
        items = [rng.randint(0, 1 << v, P2K) for _ in range(2)]
        items += [np.full(P2K, 1 << p) for p in range(v)]                              # one bit set, the same in every word
        items.append(1 << ((np.arange(P2K) * 5 + np.arange(P2K) // 126) % v))         # one bit set, moving through the positions
        items.append(np.full(P2K, (1 << v) - 1))
        x = np.array(items, np.uint8)
        return {"in": [x.reshape(-1)], "nitems": len(x)}
    if k == "vit":
        c = _cfg(po, case)
        nbytes = case["nblocks"] * 768 * c.k // 8
        data = rng.randint(0, 256, nbytes).astype(np.uint8)
        sym = np.zeros(nbytes * 8 * c.n // (c.k * c.m) + 8, np.uint8)
        L.o_inner_code.restype = C.c_size_t
        n = L.o_inner_code(C.byref(c), _p(data), C.c_size_t(nbytes), _p(sym))
        sym = sym[:n]
        for b in range(c.m):
            sym ^= ((rng.rand(n) < case["ber"]).astype(np.uint8) << b).astype(np.uint8)
        nsym_blk = 768 * c.n // c.m
        return {"in": [sym], "nitems": n, "data": data, "tags": [int(round(t * nsym_blk)) for t in case["tag_blocks"]]}
    if k in ("convint", "convdeint"):
        x = rng.randint(0, 256, case["words"] * 204).astype(np.uint8)
        return {"in": [x], "nitems": len(x) // 1632 if k == "convint" else len(x)}
    if k == "rsenc":
        x = rng.randint(0, 256, case["items"] * 8 * 188).astype(np.uint8)
        x[:188] = 0                                                                    # the all-zero word
        return {"in": [x], "nitems": case["items"]}
    if k == "rsdec":
        sent, recv, errpos = rs_words(po, case["seed"])
        return {"in": [recv.reshape(-1)], "nitems": len(recv) // 8, "sent": sent, "errpos": errpos}
    if k == "disp":
        ts = po.make_ts(case["packets"], case["seed"])
        lead = rng.randint(0, 256, case["lead"]).astype(np.uint8)
        lead[lead == 0x47] = 0x46
        x = np.concatenate([lead, ts, np.full(8, 0x47, np.uint8)])                     # forecast asks for 8 bytes beyond an item
        return {"in": [x], "nitems": len(x), "ts": ts}
    if k == "descr":
        npk = case["groups"] * 8 + 8
        ts = po.make_ts(npk, case["seed"])
        d = np.zeros(npk * 188, np.uint8)
        L.o_energy_dispersal(_p(ts), _p(d), C.c_size_t(npk))
        x = d[case["phase"] * 188:][:case["groups"] * 1504].copy()
        first = ((8 - case["phase"]) % 8) * 188                                        # the first NSYNC of the stream
        if case["damage"] == "nsync":
            x[first + case["at"] * 1504] ^= 0x10                                       # one inverted sync byte corrupted
        if case["damage"] == "lost":
            a = first + 4 * 1504 - 300
            x[a:a + 5 * 1504] = rng.randint(0, 256, 5 * 1504)                          # a stretch of garbage ...
            x[a:a + 5 * 1504][x[a:a + 5 * 1504] == 0xB8] = 0xB9                        # ... without a chance NSYNC; sync regained behind it
        return {"in": [x], "nitems": case["groups"]}
    if k == "coder":
        c = _cfg(po, case)
        nbytes = 3 * (4 * P2K * c.k * c.m // (8 * c.n))                               # 12 output items; the block works in fours
        return {"in": [rng.randint(0, 256, nbytes).astype(np.uint8)], "nitems": nbytes}
    if k == "demap":
        x = demap_points(po, case)
        return {"in": [x.view(np.uint8)], "nitems": len(x) // P2K, "points": x}
    if k == "map":
        c = _cfg(po, case)
        x = np.concatenate([np.arange(c.csize), rng.randint(0, c.csize, 3 * P2K - c.csize)]).astype(np.uint8)
        return {"in": [x], "nitems": 3}
    if k == "chain":
        c = po.cfg(case["const"], case["rate"], case["mode"])
        pps = po.packets_per_superframe(c)
        iq = po.tx(c, po.make_ts(int(pps * case.get("superframes", 1.5)), case["seed"]), lead_in=900, tail=3 * c.N)
        if "gap" in case:
            a = 900 + case["gap"][0] * (c.N + c.cp)
            iq[a:a + case["gap"][1] * (c.N + c.cp)] = 0
        o = po.rx(c, iq, want=("fft",) + CHAIN_TAPS)
        return {"cfg": c, "rx": o, "nitems": len(o["fft"])}
    if k in ("demod", "refsig"):
        cell = case.get("cell", (0, 0))
        c = po.cfg(case["const"], case["rate"], case["mode"], include_cell_id=cell[0], cell_id=cell[1])
        nsym = case["nsf"] * 272 if k == "demod" else case["nsym"]
        npk = -(-nsym * (c.payload * c.m * c.k // c.n) // (204 * 8)) + 1
        F = po.tx(c, po.make_ts(npk, case["seed"]), want_freq=True)[1][:nsym].copy()  # the generator's frequency-domain symbols: ideal FFT output
        if k == "refsig":
            return {"F": F, "nitems": nsym, "cfg": c}
        tps = c.zeros_left + np.array([c.tps[i] for i in range(c.n_tps)])
        for sym, nbits in case.get("tps_flip", ()):
            # DBPSK over the symbols of a frame: negating the TPS carriers from `sym` to the frame's end flips bit `sym` alone; negating them in one symbol flips two
            end = (sym // 68 + 1) * 68 if nbits == 1 else sym + 1
            F[sym:end, tps] *= -1
        if case.get("drop") is not None:
            F = np.delete(F, case["drop"], axis=0)
        F = np.ascontiguousarray(F[case["start"]:case["start"] + case["nfeed"]])
        return {"in": [F.reshape(-1).view(np.uint8)], "nitems": len(F), "F": F, "cfg": c}
    raise KeyError(k)


def refsig_payload(case, inp, which="ref"):
    """reference_signals' input for the case: the payload cells of the generator's symbols inp["F"], read where THE REFERENCE BLOCK puts payload -- found by a run
    of its own over cells that carry their own number -- so that its output must be the generator's symbols, pilots and TPS included, bit for bit"""
    c = inp["cfg"]
    P, N, n = c.payload, c.N, inp["nitems"]
    mark = np.zeros((n, P), np.complex64)
    mark.real = 1000 + np.arange(P)
    mark.imag = 7
    r = _refsig_block(case, c, which).stream([mark.reshape(-1).view(np.uint8)], n, [n])
    out = r["out"][0].view(np.complex64).reshape(n, N)
    pos = np.zeros((n, P), np.int64)
    for s in range(n):
        w = np.flatnonzero(out[s].imag == 7)
        assert len(w) == P and (out[s, w].real == 1000 + np.arange(P)).all()
        pos[s] = w
    return np.take_along_axis(inp["F"], pos, axis=1)


def _refsig_block(case, c, which="ref"):
    cell = case.get("cell", (0, 0))
    return rb.Block("reference_signals", [8, c.payload, c.N, case["const"], 0, case["rate"], case["rate"], 0, case["mode"], cell[0], cell[1]], which=which)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------------
def lp_undefined_mask():
    """bits of the hierarchical 64-QAM LP output of one 126-word block that the reference reads from behind its bit matrix (undefined behaviour): LP bit k
    (k = 2, 3; byte value bit 3 - k) of word i comes from row d_perm[6 i + k], column (6 i + k) / 4 of a [6][126] matrix -- outside it where row 5 meets a column >= 126"""
    m = np.zeros(126, np.uint8)
    for i in range(126):
        for k in (2, 3):
            x = 6 * i + k
            row = (x % 4) // 2 + 2 * (x % 2) + 2
            if row * 126 + x // 4 >= 6 * 126:
                m[i] |= 1 << (3 - k)
    return m


def _mask_lp(case, a):
    if case["kind"] == "bitdeint" and case["const"] == 2 and case["hier"] != 0:
        # such a bit is whatever byte lies there, not 0 or 1, and is shifted through the word: the whole byte is undefined
        return np.where(np.tile(lp_undefined_mask(), len(a) // 126) != 0, 0, a).astype(np.uint8)
    return a


def run_ref(case, inp, which="ref"):
    """drive the case's block(s) of library `which` (refblocks.lib: "ref" the reference's own blocks, "hip" the project's GNU Radio shells, which need a GPU)"""
    k = case["kind"]

    class rb:                                                                          # refblocks.Block of the library asked for
        @staticmethod
        def Block(*a, **kw):
            return _refblocks.Block(*a, which=which, **kw)
    if k == "sym":
        P = P8K if case["mode"] else P2K
        b = rb.Block("symbol_inner_interleaver", [P, case["mode"], case["direction"]])
        for i, s in enumerate(case["indices"]):
            b.tag(i, "symbol_index", s)
        return b.stream(inp["in"], inp["nitems"], case["calls"])
    if k == "bitdeint":
        b = rb.Block("bit_inner_deinterleaver", [P2K, case["const"], case["hier"], 0], nout=2)
        r = b.stream(inp["in"], inp["nitems"], case["calls"])
        if case["hier"] == 0:
            r["out"] = r["out"][:1]                                                    # the block does not write its second output
        else:
            r["out"][1] = _mask_lp(case, r["out"][1])
        return r
    if k == "bitint":
        b = rb.Block("bit_inner_interleaver", [P2K, case["const"], 0, 0], nin=2)
        return b.stream(inp["in"] * 2, inp["nitems"], case["calls"])
    if k == "vit":
        c_k = (1, 2, 3, 5, 7)[case["rate"]]
        b = rb.Block("viterbi_decoder", [case["const"], 0, case["rate"], 768, 0, 0])
        for t in inp["tags"]:
            b.tag(t, "superframe_start", 0xaa)
        return b.stream(inp["in"], inp["nitems"], [n * 768 * c_k // 8 for n in case["calls"]])
    if k == "convint":
        b = rb.Block("convolutional_interleaver", [136, 12, 17])
        return b.stream(inp["in"], inp["nitems"], [n * 1632 for n in case["calls"]])
    if k == "convdeint":
        b = rb.Block("convolutional_deinterleaver", [136, 12, 17])
        for t in case["tags"]:
            b.tag(t, "superframe_start", 1)
        return b.stream(inp["in"], inp["nitems"], case["calls"])
    if k == "rsenc":
        return rb.Block("reed_solomon_enc", RS_ARGS).stream(inp["in"], inp["nitems"], case["calls"])
    if k == "rsdec":
        return rb.Block("reed_solomon_dec", RS_ARGS).stream(inp["in"], inp["nitems"], case["calls"])
    if k == "disp":
        return rb.Block("energy_dispersal", [1]).stream(inp["in"], inp["nitems"], case["calls"], pad_items=4096)
    if k == "descr":
        # the regime oracle/o_chain.c states: the smallest call (4 items' worth of output), 4 items visible, 2 consumed ...
        r = rb.Block("energy_descramble", [1]).stream(inp["in"], inp["nitems"], [4 * 1504], visible=4)
        # ... and the same stream in calls three times as large (12 items visible, 10 consumed)
        big = rb.Block("energy_descramble", [1]).stream(inp["in"], inp["nitems"], [12 * 1504], visible=12)
        r["out"].append(big["out"][0])
        r["log_big"] = big["log"]
        n = min(len(r["out"][0]), len(big["out"][0]))
        r["big_equals_small"] = bool(n > 0 and (r["out"][0][:n] == big["out"][0][:n]).all())
        r["hints"]["forecast"] = sorted(r["hints"]["forecast"] + big["hints"]["forecast"])
        return r
    if k == "coder":
        b = rb.Block("inner_coder", [1, P2K, case["const"], case["hier"], case["rate"]])
        return b.stream(inp["in"], inp["nitems"], case["calls"])
    if k == "demap":
        return rb.Block("dvbt_demap", [P2K, case["const"], case["hier"], 0], gain=1.0).stream(inp["in"], inp["nitems"], case["calls"])
    if k == "map":
        return rb.Block("dvbt_map", [P2K, case["const"], case["hier"], 0], gain=1.0).stream(inp["in"], inp["nitems"], case["calls"])
    if k == "demod":
        c = inp["cfg"]
        b = rb.Block("demod_reference_signals", [8, c.N, c.payload, case["const"], 0, case["rate"], case["rate"], 0, case["mode"], 0, 0])
        for t in case["sync"]:
            b.tag(t, "sync_start", 1)
        return b.stream(inp["in"], inp["nitems"], [1])
    if k == "chain":
        c, o = inp["cfg"], inp["rx"]
        P, m = c.payload, case["mode"]
        b = rb.Block("demod_reference_signals", [8, c.N, P, case["const"], 0, case["rate"], case["rate"], 0, m, 0, 0])
        for j in np.flatnonzero(o["sync_flag"]):
            b.tag(int(j), "sync_start", 1)
        eq = b.stream([o["fft"].reshape(-1).view(np.uint8)], inp["nitems"], [1])
        n = len(eq["out"][0]) // (8 * P)
        demap = rb.Block("dvbt_demap", [P, case["const"], 0, m], gain=1.0).stream(eq["out"], n, [1])
        b = rb.Block("symbol_inner_interleaver", [P, m, 0])
        for _, off, key, val in eq["tags"]:
            if key == "symbol_index":
                b.tag(off, key, val)
        symd = b.stream(demap["out"], n, [1])
        bitd = rb.Block("bit_inner_deinterleaver", [P, case["const"], 0, m], nout=2).stream(symd["out"], n, [1])
        b = rb.Block("viterbi_decoder", [case["const"], 0, case["rate"], 768, 0, 0])
        for _, off, key, val in eq["tags"]:
            if key == "superframe_start":
                b.tag(off * P, key, val)                                                # the tag travels with its item through the three 1:1 blocks
        vit = b.stream(bitd["out"][:1], n * P, [768 * c.k // 8])
        b = rb.Block("convolutional_deinterleaver", [136, 12, 17])
        for _, off, key, val in vit["tags"]:
            b.tag(off, key, val)
        dei = b.stream(vit["out"], len(vit["out"][0]), [2])
        rs = rb.Block("reed_solomon_dec", RS_ARGS).stream(dei["out"], len(dei["out"][0]) // 1632, [1])
        ts = rb.Block("energy_descramble", [1]).stream(rs["out"], len(rs["out"][0]) // 1504, [4 * 1504], visible=4)
        outs = [r["out"][0] for r in (eq, demap, symd, bitd, vit, dei, rs, ts)]
        # o_rx_run's Viterbi tap is the decoder's output without the bytes that the byte de-interleaver drops in front of a tag (oracle/o_chain.c): the same here
        pos, kept_bytes = 0, []
        for _, r, cons in dei["log"]:
            if r > 0:
                kept_bytes.append(outs[4][pos:pos + cons])
            pos += cons
        outs[4] = np.concatenate(kept_bytes + [outs[4][pos:]])
        return {"out": outs, "log": [[len(x), 0, 0] for x in outs], "tags": eq["tags"][:1] + vit["tags"],
                "hints": [r["hints"] for r in (eq, demap, symd, bitd, vit, dei, rs, ts)]}
    if k == "refsig":
        c = inp["cfg"]
        pay = refsig_payload(case, inp, which)
        return _refsig_block(case, c, which).stream([pay.reshape(-1).view(np.uint8)], inp["nitems"], case["calls"])
    raise KeyError(k)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the oracle, in the same calls
# ------------------------------------------------------------------------------------------------------------------------------------------
def _tagged_stream(nitems, calls, tags, in_per_out):
    """convolutional_deinterleaver's reaction to a tag (convolutional_deinterleaver_impl.cc:109-120; viterbi_decoder_impl.cc:213-229 is the same, laid out in blocks
    in run_oracle): a call that finds a superframe_start tag in the input it is about to take, not at its first item, consumes up to the tag and returns 0.
    yields (noutput, first input item, input items taken or None for such a call, tag seen)"""
    pos, ci = 0, 0
    while True:
        n = calls[min(ci, len(calls) - 1)]
        need = n * in_per_out
        if pos + need > nitems:
            return
        seen = [t for t in sorted(tags) if pos <= t < pos + need]
        if seen and seen[0] != pos:
            yield n, pos, None, True
            pos = seen[0]
        else:
            yield n, pos, need, bool(seen)
            pos += need
        ci += 1


def run_oracle(po, case, inp):
    k = case["kind"]
    L = po.lib()
    x = inp["in"][0] if "in" in inp else None
    if k == "sym":
        c = po.cfg(1, 0, case["mode"])
        P = c.payload
        H = np.zeros(P, np.int32)
        L.o_sym_H(C.byref(c), _p(H))
        out = np.zeros(inp["nitems"] * P, np.uint8)
        log = _log_1to1(inp["nitems"], case["calls"])
        done = sum(e[2] for e in log)
        for i in range(done):
            si = case["indices"][i] if case["direction"] == 0 else i % 68
            L.o_sym_interleave(C.byref(c), _p(H), _p(x[i * P:]), _p(out[i * P:]), si, case["direction"])
        return {"out": [out[:done * P]], "log": log, "tags": []}
    if k in ("bitdeint", "bitint"):
        c = _cfg(po, case)
        log = _log_1to1(inp["nitems"], case["calls"])
        n = sum(e[2] for e in log) * P2K
        o0, o1 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        if k == "bitint":
            L.o_bit_interleave(C.byref(c), _p(x), _p(o0), C.c_size_t(n))
            outs = [o0]
        elif case["hier"] == 0:
            L.o_bit_deinterleave(C.byref(c), _p(x), _p(o0), C.c_size_t(n))
            outs = [o0]
        else:
            L.o_bit_deinterleave_hier(C.byref(c), _p(x), _p(o0), _p(o1), C.c_size_t(n))
            outs = [o0, _mask_lp(case, o1)]
        return {"out": outs, "log": log, "tags": []}
    if k == "vit":
        c = _cfg(po, case)
        nsym_blk, nout_blk, ntb = 768 * c.n // c.m, 768 * c.k // 8, L.o_vit_ntraceback(case["rate"])
        L.o_viterbi_decode_n.restype = C.c_size_t
        L.o_viterbi_decode_n.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        log, tags, outs, period, written, init = [], [], [], [], 0, 0

        def flush():
            if period:
                vin = np.concatenate(period)
                o = np.zeros(len(vin) * c.m * c.k // (8 * c.n) + 64, np.uint8)
                outs.append(o[:L.o_viterbi_decode_n(C.byref(c), vin.ctypes.data, len(vin), o.ctypes.data)])
                del period[:]
        pos, ci = 0, 0
        while True:
            nb = case["calls"][min(ci, len(case["calls"]) - 1)]
            need = nb * nsym_blk
            if pos + need > inp["nitems"]:
                break
            seen = [t for t in sorted(inp["tags"]) if pos <= t < pos + need]
            if seen:
                flush()                                                                # the tag resets the decoder ...
                init = 0
            if seen and seen[0] != pos:
                log.append([nb * nout_blk, 0, seen[0] - pos])                          # ... and what lies in front of it is dropped undecoded
                pos = seen[0]
            else:
                period.append(x[pos:pos + need])
                r = nb * nout_blk
                if init == 0:
                    tags.append([0, written, "superframe_start", 1])
                    r -= ntb
                    init = 1
                log.append([nb * nout_blk, r, need])
                written += r
                pos += need
            ci += 1
        flush()
        return {"out": [np.concatenate(outs) if outs else np.zeros(0, np.uint8)], "log": log, "tags": tags}
    if k == "convint":
        log = [[n * 1632, n * 1632, n] for n, _, _ in _log_1to1(inp["nitems"], case["calls"])]
        n = sum(e[2] for e in log) * 1632
        o = np.zeros(n, np.uint8)
        L.o_conv_interleave(_p(x), _p(o), C.c_size_t(n))
        return {"out": [o], "log": log, "tags": []}
    if k == "convdeint":
        log, taken = [], []
        for n, pos, take, _ in _tagged_stream(inp["nitems"], case["calls"], case["tags"], 1632):
            if take is None:
                nxt = [t for t in sorted(case["tags"]) if t > pos][0]
                log.append([n, 0, nxt - pos])
            else:
                log.append([n, n, take])
                taken.append(x[pos:pos + take])
        vin = np.concatenate(taken) if taken else np.zeros(0, np.uint8)
        if case["calls"] == [2]:
            # the regime oracle/o_chain.c states (one pair of items per call): what is taken in front of a tag is the oracle's own rule, not the layout above
            L.o_conv_deint_taken_before_tag.restype = C.c_size_t
            L.o_conv_deint_taken_before_tag.argtypes = [C.c_size_t]
            edges = sorted(set([0] + [t for t in case["tags"] if t > 0]))
            parts = [x[a:a + L.o_conv_deint_taken_before_tag(b - a)] for a, b in zip(edges[:-1], edges[1:])]
            parts.append(x[edges[-1]:edges[-1] + (inp["nitems"] - edges[-1]) // 3264 * 3264])
            vin = np.concatenate(parts)
        o = np.zeros(len(vin), np.uint8)
        L.o_conv_deinterleave(_p(vin), _p(o), C.c_size_t(len(vin)))                    # the FIFOs go on across the tag: one stream of what was taken
        return {"out": [o], "log": log, "tags": []}
    if k == "rsenc":
        rs = po.RS()
        L.o_rs_init(C.byref(rs))
        log = _log_1to1(inp["nitems"], case["calls"])
        nw = sum(e[2] for e in log) * 8
        o = np.zeros((nw, 204), np.uint8)
        for i in range(nw):
            w = np.zeros(255, np.uint8)
            w[51:239] = x[i * 188:(i + 1) * 188]
            L.o_rs_encode(C.byref(rs), _p(w), _p(w[239:]))
            o[i] = w[51:]
        return {"out": [o.reshape(-1)], "log": log, "tags": []}
    if k == "rsdec":
        return {"out": [rs_decode(po, x, inp["nitems"] * 8, 1)], "log": _log_1to1(inp["nitems"], case["calls"]), "tags": []}
    if k == "disp":
        # the block looks for the first sync byte (0x47) within 188 bytes of every call's start, then takes whole items of 8 packets
        o = np.zeros(case["packets"] * 188, np.uint8)
        L.o_energy_dispersal(_p(inp["ts"]), _p(o), C.c_size_t(case["packets"]))
        nitems_out = sum(e[0] for e in _log_1to1(case["packets"] // 8, case["calls"]))
        return {"out": [o[:nitems_out * 1504]], "log": None, "tags": []}
    if k == "descr":
        o = np.zeros(inp["nitems"] * 1504, np.uint8)
        n = L.o_energy_descramble(_p(x), C.c_size_t(inp["nitems"]), _p(o))
        return {"out": [o[:n]], "log": None, "tags": []}
    if k == "coder":
        c = _cfg(po, case)
        L.o_inner_code.restype = C.c_size_t
        per4 = 4 * P2K * c.k * c.m // (8 * c.n)                                        # inner_coder_impl.cc:208,258
        log = [[n, n, n // 4 * per4] for n, _, _ in _log_1to1(inp["nitems"] * 4 // per4, case["calls"])]
        nbytes = sum(e[2] for e in log)
        o = np.zeros(nbytes * 8 * c.n // (c.k * c.m) + 8, np.uint8)
        n = L.o_inner_code(C.byref(c), _p(x), C.c_size_t(nbytes), _p(o))
        return {"out": [o[:n]], "log": log, "tags": []}
    if k in ("demap", "map"):
        c = _cfg(po, case)
        pts = np.zeros(c.csize, np.complex64)
        L.o_constellation(C.byref(c), C.c_float(1.0), _p(pts))
        log = _log_1to1(inp["nitems"], case["calls"])
        n = sum(e[2] for e in log) * P2K
        if k == "map":
            return {"out": [pts[x[:n]].view(np.uint8)], "log": log, "tags": []}
        o = np.zeros(n, np.uint8)
        L.o_demap(C.byref(c), _p(pts), _p(inp["points"]), _p(o), C.c_size_t(n))
        return {"out": [o], "log": log, "tags": []}
    if k == "demod":
        c = inp["cfg"]
        F = inp["F"]
        L.o_demod_new.restype = C.c_void_p
        d = C.c_void_p(L.o_demod_new(C.byref(c)))
        log, tags, outs, written = [], [], [], 0
        sf, si = C.c_int(), C.c_int()
        info = (C.c_int * 8)()
        buf = np.concatenate([F.reshape(-1), np.zeros(c.N, np.complex64)])
        for j in range(inp["nitems"] - 1):                                             # forecast: two items visible
            o = np.zeros(c.payload, np.complex64)
            r = L.o_demod_work(d, _p(buf[j * c.N:]), _p(o), int(j in case["sync"]), C.byref(sf), C.byref(si), info)
            if sf.value:
                tags.append([0, written, "superframe_start", 0xaa])
            if r:
                tags.append([0, written, "symbol_index", si.value])
                outs.append(o)
            log.append([1, r, 1])
            written += r
        L.o_demod_free(d)
        out = np.concatenate(outs) if outs else np.zeros(0, np.complex64)
        return {"out": [out.view(np.uint8)], "log": log, "tags": tags}
    if k == "chain":
        # o_rx_run with the default Reed-Solomon mode: on a clean loopback no word needs correcting, so it equals the reference's
        o = inp["rx"]
        outs = [np.ascontiguousarray(o[t]).reshape(-1).view(np.uint8) for t in CHAIN_TAPS]
        return {"out": outs, "log": None, "tags": None}
    if k == "refsig":
        n = sum(e[2] for e in _log_1to1(inp["nitems"], case["calls"]))
        return {"out": [np.ascontiguousarray(inp["F"][:n]).reshape(-1).view(np.uint8)], "log": _log_1to1(inp["nitems"], case["calls"]), "tags": []}
    raise KeyError(k)


def rs_decode(po, recv, nwords, compat):
    L = po.lib()
    rs = po.RS()
    L.o_rs_init(C.byref(rs))
    L.o_rs_dec_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    o = np.zeros(nwords * 188, np.uint8)
    L.o_rs_dec_block(C.byref(rs), _p(recv), _p(o), nwords, compat, None, None)
    return o


def record(res):
    """what is kept of a run in tests/golden/ref_blocks.json: counts, tags and a SHA-256 per output"""
    r = {"log": rle(res["log"]), "tags": rle(res["tags"]), "sha256": [sha(o) for o in res["out"]], "nbytes": [int(len(o)) for o in res["out"]]}
    for key in ("log_big", "big_equals_small"):
        if key in res:
            r[key] = rle(res[key]) if key == "log_big" else res[key]
    return r


def sched(res):
    """what the block(s) of a run asked of the scheduler (refblocks.Block.hints; a list, block by block, for the chain cases): the recording keeps it as its key `sched`"""
    return res["hints"]


def kept(case, res):
    """the float values of a reference run that go into tests/golden/ref_blocks.npz for the GPU tests: {key: (byte offset in output 0, complex64 values)}"""
    k = case["kind"]
    out = res["out"][0]
    if k == "map":
        return {case["name"] + "_first512": (0, out[:512 * 8].view(np.complex64).copy())}
    if k in ("demod", "refsig") and "keep" in case:
        size = 8 * (P2K if k == "demod" else 2048)
        return {"%s_item%d" % (case["name"], i): (i * size, out[i * size:(i + 1) * size].view(np.complex64).copy()) for i in case["keep"]}
    return {}


def rle(entries):
    """a list of calls or tags with runs folded, as the recording keeps it: calls [[entry, count], ...] of equal entries; tags [[tag, count, value step], ...] of tags
    on successive items whose value goes up by the step (0 or 1)"""
    out = []
    for e in entries:
        e = list(e)
        if out and len(e) == 3 and out[-1][0] == e:
            out[-1][1] += 1
            continue
        if out and len(e) == 4:
            last, n, dv = out[-1]
            if last[0] == e[0] and last[2] == e[2] and last[1] + n == e[1] and (e[3] - last[3] == dv * n or (n == 1 and e[3] - last[3] in (0, 1))):
                out[-1][2] = e[3] - last[3] if n == 1 else dv
                out[-1][1] += 1
                continue
        out.append([e, 1] if len(e) == 3 else [e, 1, 0])
    return out


def unrle(folded):
    out = []
    for f in folded:
        for i in range(f[1]):
            x = list(f[0])
            if len(x) == 4:
                x[1] += i
                x[3] += i * f[2]
            out.append(x)
    return out
