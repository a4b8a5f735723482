"""The ten receive blocks of the per-block C ABI, each through dvbt_<blk>_work (host buffers) and dvbt_<blk>_work_device (torch device buffers on one
stream), across the configurations and call sizes where kernels go wrong: every mode and guard, every constellation and hierarchy, every code rate,
demapper gains that stretch or switch off the grid fast path, the 4096-item and 64-slot limits, streams split over calls of 1 to 1000 items, and RS
corpora that drive either decoder of reed_solomon_dec.  The two entries must agree exactly, a split stream must equal one call, and both must equal
the oracle (oracle/) or a plain restatement (tests/rxref.py).  Integer outputs are compared bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rxref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_DEROT = 2e-4          # tests/test_gpu_channel.py: acquisition items on a channel, after one rotation per item


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    return gr_dvbt_amd


@pytest.fixture(scope="module")
def dev():
    """device-buffer calls on one HIP stream: inputs go up, outputs come back after the stream has drained"""
    import torch

    class Dev:
        def __init__(self):
            self.torch = torch
            self.s = torch.cuda.Stream()

        def up(self, a):
            with torch.cuda.stream(self.s):
                return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda", non_blocking=False)

        def buf(self, nbytes):
            with torch.cuda.stream(self.s):
                return torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")

        def call(self, b, nout, nin, x, out_bytes, tags=()):
            """one work_device call on a fresh copy of x; returns (produced, consumed, tags, output bytes)"""
            xin, out = self.up(x), self.buf(out_bytes)
            r, cons, tout = b.work_device(nout, nin, xin.data_ptr(), out.data_ptr(), tags, self.s.cuda_stream)
            self.s.synchronize()
            return r, cons, tout, out[:out_bytes].cpu().numpy()
    return Dev()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _call(entry, dev, b, nout, nin, x, out_bytes, tags=()):
    if entry == "host":
        out = np.zeros(out_bytes, np.uint8)
        r, cons, tout = b.work(nout, nin, np.ascontiguousarray(x), out, tags)
        return r, cons, tout, out
    return dev.call(b, nout, nin, x, out_bytes, tags)


ENTRIES = ("host", "device")


# ---------------------------------------------------------------- A1 ofdm_sym_acquisition
def _unrotate(a, b):
    ph = (a * np.conj(b)).sum(axis=1)
    ph = ph / np.maximum(np.abs(ph), 1e-30)
    return b * ph[:, None]


ACQ = [(m, gi, 0.0) for m in (0, 1) for gi in range(4)] + [(0, 1, -5.37), (1, 2, 7.2)]


@pytest.mark.parametrize("mode,guard,cfo", ACQ, ids=[f"{'28'[m]}k-g{gi}-cfo{cfo}" for m, gi, cfo in ACQ])
def test_acquisition(po, g, dev, mode, guard, cfo):
    """calls of 1, 3, 17, 64 items, each offered what forecast() asks: items as the oracle's acq tap, the sync_start tag on the first call only,
    the samples consumed as the oracle's call positions"""
    c = po.cfg(po.QAM16, po.C1_2, mode, guard=guard)
    nsym = 150 if mode == 0 else 90
    iq = po.tx(c, po.make_ts(nsym * po.packets_per_superframe(c) // 272 + 8, 8), lead_in=700, tail=3 * c.N)
    if cfo:
        iq = po.channel(iq, c.N, cfo=cfo)
    o = po.rx(c, iq, want=("acq",))
    ref, call_pos = o["acq"], o["call_pos"]
    runs = {}
    for entry in ENTRIES:
        b = g.Block("ofdm_sym_acquisition", 1, c.N, c.Kmax + 1, c.cp, 30.0)
        pos, items, k, tagged = 0, [], 0, []
        while True:
            # GNU Radio's executor asks for less when the input cannot meet the forecast (block_executor.cc): at the end of the stream
            want = min((1, 3, 17, 64)[k % 4], (len(iq) - pos - (2 * c.N + c.cp + 16)) // (c.N + c.cp) + 1)
            if want < 1:
                break
            need = b.forecast(want)
            assert need == (want - 1) * (c.N + c.cp) + 2 * c.N + c.cp + 16
            chunk = iq[pos:pos + need]
            r, cons, tags, out = _call(entry, dev, b, want, len(chunk), chunk, want * c.N * 8)
            if r == 0 and cons == 0:
                break
            if (0, g.TAG_SYNC_START, 1) in tags:
                tagged.append(sum(len(a) for a in items))               # the tag's absolute output offset
            items.append(out.view(np.complex64).reshape(want, c.N)[:r])
            pos += cons
            n = sum(len(a) for a in items)
            if r and n < len(call_pos):
                assert pos == call_pos[n], (k, pos, call_pos[n])
            k += 1
        b.close()
        runs[entry] = np.concatenate(items)
        # sync_start on the first call, and again only where the oracle re-acquired (its sync flags) or after the last item (lock lost in the tail)
        want_tags = [int(i) for i in np.flatnonzero(o["sync_flag"]) if i < len(runs[entry])]
        assert want_tags[:1] == [0] and tagged[:1] == [0]
        assert sorted({t for t in tagged if t < len(runs[entry])}) == want_tags, (entry, tagged, want_tags)
    got = runs["host"]
    assert got.shape == runs["device"].shape and (got.view(np.uint32) == runs["device"].view(np.uint32)).all()
    n = min(len(got), len(ref))
    assert n >= 0.85 * len(ref), (n, len(ref))
    if cfo:
        err = np.abs(_unrotate(got[:n], ref[:n]) - got[:n]).max() / np.abs(got[:n]).max()
        tol = TOL_DEROT
    else:
        err = np.abs(got[:n] - ref[:n]).max() / np.abs(ref).max()
        tol = 1e-6
    print(f"\n[acq {'28'[mode]}k guard {guard} cfo {cfo}] {n} items, error {err:.2e} of the peak")
    assert err <= tol


# ---------------------------------------------------------------- A3 demod_reference_signals
DEMOD = [(m, gi, const, 0, (3 * m + gi + const) % 5, (m + gi + const) % 2) for m in (0, 1) for gi in range(4) for const in range(3)]
DEMOD += [(0, 1, 1, 2, 1, 0), (1, 0, 2, 3, 2, 1)]                  # hierarchical alpha = 2 and 4


@pytest.mark.parametrize("mode,guard,const,hier,cr,cid", DEMOD, ids=[f"{'28'[a[0]]}k-g{a[1]}-c{a[2]}-h{a[3]}-r{a[4]}-cid{a[5]}" for a in DEMOD])
def test_demod(po, g, dev, mode, guard, const, hier, cr, cid):
    """calls of 1, 5, 100, 300 items over the oracle's FFT items: equalised carriers within the contract's tolerance, the superframe_start tag on
    the oracle's first output symbol, one symbol_index tag per item.  The LP rate the block is given differs from the HP rate (the receiver does
    not use it)."""
    cell = 0x5a if cid else 0
    c = po.cfg(const, cr, mode, guard=guard, hierarchy=hier, include_cell_id=cid, cell_id=cell)
    pps = po.packets_per_superframe(c)
    iq = po.tx(c, po.make_ts(pps + pps // 2, 9), lead_in=900, tail=3 * c.N)
    o = po.rx(c, iq, want=("fft", "eq"))
    fft, fo = o["fft"], o["first_out_symbol"]
    assert fo >= 0 and len(o["eq"]) > 50
    runs = {}
    for entry in ENTRIES:
        b = g.Block("demod_reference_signals", 8, c.N, c.payload, const, hier, cr, (cr + 2) % 5, guard, mode, cid, cell)
        pos, outs, all_tags, produced, k = 0, [], [], 0, 0
        while True:
            want = (1, 5, 100, 300)[k % 4]
            k += 1
            avail = min(want + 1, len(fft) - pos)
            if avail < 2:
                break
            r, cons, tags, out = _call(entry, dev, b, want, avail, fft[pos:pos + avail], want * c.payload * 8,
                                       tags=[(0, g.TAG_SYNC_START, 1)] if pos == 0 else [])
            assert cons == avail - 1
            all_tags += [(off + produced, key, v) for off, key, v in tags]
            outs.append(out.view(np.complex64).reshape(want, c.payload)[:r])
            produced += r
            pos += cons
        b.close()
        runs[entry] = (np.concatenate(outs), all_tags)
    got, all_tags = runs["host"]
    assert (got.view(np.uint32) == runs["device"][0].view(np.uint32)).all() and all_tags == runs["device"][1]
    n = min(len(got), len(o["eq"]))
    assert n > 0.9 * len(o["eq"]) and n > 50
    d = got[:n] - o["eq"][:n]
    assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= 1e-3 * 2 * c.norm
    assert [t for t in all_tags if t[1] == g.TAG_SUPERFRAME_START] == [(0, g.TAG_SUPERFRAME_START, 0xaa)]
    si = [t for t in all_tags if t[1] == g.TAG_SYMBOL_INDEX]
    assert [t[0] for t in si] == list(range(len(got)))
    assert [t[2] for t in si][:n] == list(o["sym_index"][fo:fo + n])


# ---------------------------------------------------------------- A4 dvbt_demap
DEMAP = [(const, hier, m) for const, hier in [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3)] for m in (0, 1)]
GAINS = (1.0, 0.5, 2.0, 1.0 / 64, 64.0, -1.0)


def _demap_carriers(c, pts, gain, rng):
    s = abs(gain) * c.norm
    x = [pts, (pts + np.roll(pts, 1)) / 2, (pts + np.roll(pts, 3)) / 2,                                     # exact points and midpoints
         ((rng.rand(400) - 0.5) + 1j * (rng.rand(400) - 0.5)) * 2 * c.alpha * s,                          # the centre gap
         (rng.randn(400) + 1j * rng.randn(400)) * 40 * abs(gain),     # far outside the grid (scaled with the gain: at 40 / 64 units out the nearest
                                                                      # points' distances differ by less than a float32 ulp, and either is right)
         pts[rng.randint(0, c.csize, 1000)] + 0.45 * s * (rng.randn(1000) + 1j * rng.randn(1000))]
    sweep = np.linspace(-12 * s, 12 * s, 600)
    x += [sweep + 1j * 0.3 * s, -1.7 * s + 1j * sweep]                                                   # across every decision boundary of one axis
    return np.concatenate(x).astype(np.complex64)


@pytest.mark.parametrize("const,hier,mode", DEMAP)
def test_demap(po, g, dev, const, hier, mode):
    """every gain, each at one of the item sizes 1, 1000, payload, 49152 (rotated): labels bit-exact against o_demap on the oracle's constellation
    at that gain"""
    c = po.cfg(const, po.C1_2, mode, hierarchy=hier)
    rng = np.random.RandomState(20 + 3 * const + hier + 11 * mode)
    sizes = (1, 1000, c.payload, 49152)
    for gi, gain in enumerate(GAINS):
        pts = np.zeros(c.csize, np.complex64)
        po.lib().o_constellation(C.byref(c), C.c_float(gain), _p(pts))
        x = _demap_carriers(c, pts, gain, rng)
        nsize = sizes[(gi + const + hier + mode) % 4]
        if nsize == 1:
            x = x[:800]
        n = -(-len(x) // nsize)
        pad = pts[rng.randint(0, c.csize, n * nsize - len(x))] + 0.3 * abs(gain) * c.norm * rng.randn(n * nsize - len(x))
        x = np.concatenate([x, pad.astype(np.complex64)])
        ref = np.zeros(len(x), np.uint8)
        po.lib().o_demap(C.byref(c), _p(pts), _p(x), _p(ref), C.c_size_t(len(x)))
        b = g.Block("demap", nsize, const, hier, mode, gain)
        for entry in ENTRIES:
            r, cons, _, out = _call(entry, dev, b, n, n, x, n * nsize)
            assert r == n and cons == n
            assert (out == ref).all(), (gain, nsize, entry, np.flatnonzero(out != ref)[:5])
        b.close()


# ---------------------------------------------------------------- A5 symbol_inner_interleaver, RX direction
def _sym_perms(po, c):
    """the de-interleaver's gather for even and odd symbol indices, read off o_sym_interleave (direction 0) applied to the carrier numbers"""
    H = np.zeros(c.payload, np.int32)
    po.lib().o_sym_H(C.byref(c), _p(H))
    q = np.arange(c.payload)
    perms = []
    for si in (0, 1):
        lo, hi = (q & 0xff).astype(np.uint8), (q >> 8).astype(np.uint8)
        a, b = np.zeros_like(lo), np.zeros_like(hi)
        po.lib().o_sym_interleave(C.byref(c), _p(H), _p(lo), _p(a), si, 0)
        po.lib().o_sym_interleave(C.byref(c), _p(H), _p(hi), _p(b), si, 0)
        perms.append(a.astype(np.int64) | (b.astype(np.int64) << 8))
    return H, perms


@pytest.mark.parametrize("mode", [0, 1])
def test_symbol_deinterleaver(po, g, dev, mode):
    c = po.cfg(po.QAM16, po.C1_2, mode)
    P = c.payload
    H, perms = _sym_perms(po, c)
    rng = np.random.RandomState(30 + mode)
    b = g.Block("symbol_inner_interleaver", P, mode, 0)
    # every one of the 68 symbol indices, in one call of 68 items (shuffled tags), against o_sym_interleave itself
    idx = rng.permutation(68)
    x = rng.randint(0, 64, (68, P)).astype(np.uint8)
    ref = np.zeros_like(x)
    for i, si in enumerate(idx):
        po.lib().o_sym_interleave(C.byref(c), _p(H), _p(x[i]), _p(ref[i]), int(si), 0)
        assert (ref[i] == x[i][perms[si % 2]]).all()
    for entry in ENTRIES:
        r, cons, _, out = _call(entry, dev, b, 68, 68, x, 68 * P, tags=[(i, g.TAG_SYMBOL_INDEX, int(si)) for i, si in enumerate(idx)])
        assert r == cons == 68 and (out.reshape(68, P) == ref).all(), entry
    # calls of 1 and of 4096 items (the cap); 4097 is refused by both entries
    for n in (1, 1, 4096):
        idx = rng.randint(0, 68, n)
        x = rng.randint(0, 64, (n, P)).astype(np.uint8)
        ref = np.stack([x[i][perms[si % 2]] for i, si in enumerate(idx)])
        tags = [(i, g.TAG_SYMBOL_INDEX, int(si)) for i, si in enumerate(idx)]
        for entry in ENTRIES:
            r, cons, _, out = _call(entry, dev, b, n, n, x, n * P, tags=tags)
            assert r == cons == n and (out.reshape(n, P) == ref).all(), (n, entry)
    x = np.zeros((4097, P), np.uint8)
    tags = [(i, g.TAG_SYMBOL_INDEX, i % 68) for i in range(4097)]
    with pytest.raises(g.DvbtError):
        b.work(4097, 4097, x, np.zeros_like(x), tags)
    xin, out = dev.up(x), dev.buf(x.size)
    with pytest.raises(g.DvbtError):
        b.work_device(4097, 4097, xin.data_ptr(), out.data_ptr(), tags, dev.s.cuda_stream)
    dev.s.synchronize()
    b.close()
    # more than 64 device calls queued on one stream before anything is waited for: every call's index table needs its own slot of the ring
    b = g.Block("symbol_inner_interleaver", P, mode, 0)
    ncalls, sizes = 150, rng.randint(1, 4, 150)
    x = rng.randint(0, 64, (int(sizes.sum()), P)).astype(np.uint8)
    idx = rng.randint(0, 68, len(x))
    xin, out = dev.up(x), dev.buf(x.size)
    pos = 0
    for k in range(ncalls):
        n = int(sizes[k])
        tags = [(i, g.TAG_SYMBOL_INDEX, int(idx[pos + i])) for i in range(n)]
        r, cons, _ = b.work_device(n, n, xin.data_ptr() + pos * P, out.data_ptr() + pos * P, tags, dev.s.cuda_stream)
        assert r == cons == n
        pos += n
    dev.s.synchronize()
    got = out[:x.size].cpu().numpy().reshape(-1, P)
    ref = np.stack([x[i][perms[si % 2]] for i, si in enumerate(idx)])
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert len(bad) == 0, bad[:10]
    b.close()


# ---------------------------------------------------------------- A6 bit_inner_deinterleaver
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("const", [0, 1, 2])
def test_bit_deinterleaver(po, g, dev, const, mode):
    c = po.cfg(const, po.C1_2, mode)
    rng = np.random.RandomState(40 + const + 3 * mode)
    for nsize in (126, 252, c.payload, 49140):
        n = {126: 37, 252: 11, 49140: 2}.get(nsize, 3)
        x = rng.randint(0, c.csize, n * nsize).astype(np.uint8)
        ref = np.zeros_like(x)
        po.lib().o_bit_deinterleave(C.byref(c), _p(x), _p(ref), C.c_size_t(x.size))
        b = g.Block("bit_inner_deinterleaver", nsize, const, 0, mode)
        for entry in ENTRIES:
            r, cons, _, out = _call(entry, dev, b, n, n, x, x.size)
            assert r == cons == n and (out == ref).all(), (nsize, entry)
        b.close()


@pytest.mark.parametrize("const,hier", [(1, 1), (1, 3), (2, 2), (2, 3)])
def test_bit_deinterleaver_hierarchical_8k(po, g, dev, const, hier):
    c = po.cfg(const, po.C1_2, po.T8k, hierarchy=hier)
    L = g.lib()
    L.dvbt_bit_inner_deinterleaver_work_hier.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dvbt_bit_inner_deinterleaver_work_hier_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.RandomState(50 + hier)
    for nsize in (c.payload, 252):
        n = 3 if nsize == c.payload else 9
        x = rng.randint(0, c.csize, n * nsize).astype(np.uint8)
        rh, rl = np.zeros_like(x), np.zeros_like(x)
        po.lib().o_bit_deinterleave_hier(C.byref(c), _p(x), _p(rh), _p(rl), C.c_size_t(x.size))
        b = g.Block("bit_inner_deinterleaver", nsize, const, hier, po.T8k)
        oh, ol = np.zeros_like(x), np.full_like(x, 0xee)
        assert L.dvbt_bit_inner_deinterleaver_work_hier(b.h, n, n, _p(x), _p(oh), _p(ol), None) == n
        assert (oh == rh).all() and (ol == rl).all()
        xin, dh, dl = dev.up(x), dev.buf(x.size), dev.buf(x.size)
        assert L.dvbt_bit_inner_deinterleaver_work_hier_device(b.h, n, n, xin.data_ptr(), dh.data_ptr(), dl.data_ptr(), None, dev.s.cuda_stream) == n
        dev.s.synchronize()
        assert (dh[:x.size].cpu().numpy() == rh).all() and (dl[:x.size].cpu().numpy() == rl).all()
        r, cons, _, out = _call("device", dev, b, n, n, x, x.size)                   # the one-output entry: port 0
        assert r == n and (out == rh).all()
        b.close()


# ---------------------------------------------------------------- A7 viterbi_decoder
VIT = [(const, cr, 0) for const in range(3) for cr in range(5)] + [(1, 1, 2), (2, 3, 3)]


@pytest.mark.parametrize("const,cr,hier", VIT, ids=[f"c{a}-r{b}-h{h}" for a, b, h in VIT])
def test_viterbi(po, g, dev, const, cr, hier):
    """bsize 768 and 48 (legal in every mode), calls split down to one reference block, host and device entries alternating on one handle:
    the bytes of o_viterbi_decode (pinned to the reference's own kernels).  hier > 0: the HP decode of a hierarchical mode."""
    c = po.cfg(const, cr, po.T2k, hierarchy=hier)
    ntb = g.get_dims(const, cr, po.T2k, hierarchy=hier).ntraceback
    for bsize, nblocks in ((768, 23), (48, 300)):
        d_nsym, d_nout = bsize * c.n // c.m, bsize * c.k // 8
        ber = (0.0, 0.01, 0.004)[(const + cr + bsize) % 3]
        data, sym = rxref.coded_symbols(po, c, d_nout * nblocks + 64, ber, 60 + 5 * const + cr + bsize)
        sym = sym[:d_nsym * nblocks].copy()
        ref = np.zeros(d_nout * nblocks + 64, np.uint8)
        n_ref = po.lib().o_viterbi_decode(C.byref(c), bsize, _p(sym), len(sym), _p(ref))
        assert n_ref == d_nout * nblocks - ntb
        if ber == 0.0 and hier == 0:
            assert (ref[:n_ref] == data[:n_ref]).all()
        b = g.Block("viterbi_decoder", const, hier, cr, bsize, 0, -1)
        assert b.forecast(d_nout) == d_nsym
        outs, pos, k = [], 0, 0
        while pos < len(sym):
            nb = min((1, 2, 7, 1, 1, 12, 40)[k % 7], (len(sym) - pos) // d_nsym)
            entry = ENTRIES[k % 2]
            tags = [(0, g.TAG_SUPERFRAME_START, 0xaa)] if k == 0 else []
            r, cons, tout, out = _call(entry, dev, b, nb * d_nout, nb * d_nsym, sym[pos:pos + nb * d_nsym], nb * d_nout, tags)
            assert cons == nb * d_nsym and r == nb * d_nout - (ntb if k == 0 else 0), (bsize, k)
            assert (tout == [(0, g.TAG_SUPERFRAME_START, 1)]) == (k == 0)
            outs.append(out[:r])
            pos += cons
            k += 1
        b.close()
        out = np.concatenate(outs)
        assert len(out) == n_ref and (out == ref[:n_ref]).all(), (bsize, np.flatnonzero(out != ref[:n_ref])[:5])


# ---------------------------------------------------------------- A8 convolutional_deinterleaver
def test_convolutional_deinterleaver(po, g, dev):
    """calls of 2, 3 (two are taken), 82, 100 and 1000 items -- past the 131,072 bytes of the kernel's fixed grid, so the stride loop's later passes
    run -- and the same stream in one call"""
    calls = (2, 3, 82, 100, 1000)
    total = 2 + 2 + 82 + 100 + 1000
    rng = np.random.RandomState(70)
    x = rng.randint(0, 256, (total + 1) * 1632).astype(np.uint8)
    ref = np.zeros_like(x)
    po.lib().o_conv_deinterleave(_p(x), _p(ref), C.c_size_t(len(x)))
    for entry in ENTRIES:
        b = g.Block("convolutional_deinterleaver", 136, 12, 17)
        outs, pos = [], 0
        for n in calls:
            r, cons, _, out = _call(entry, dev, b, n, len(x) - pos, x[pos:], n * 1632)
            assert r == n & ~1 and cons == r * 1632
            outs.append(out[:cons])
            pos += cons
        b.close()
        got = np.concatenate(outs)
        assert len(got) == total * 1632 and (got == ref[:len(got)]).all(), (entry, np.flatnonzero(got != ref[:len(got)])[:5])
        b = g.Block("convolutional_deinterleaver", 136, 12, 17)
        r, cons, _, out = _call(entry, dev, b, total, total * 1632, x, total * 1632)
        assert r == total and (out == got).all()
        b.close()


# ---------------------------------------------------------------- A9 reed_solomon_dec
RS_CALLS = (1000, 64, 8, 3, 1)                           # items of 8 words: whole wavefronts first, then a partial one of 24 and of 8 words
RS_CASES = [(bad, compat, where) for bad, where in ((0, "random"), (1, "first"), (23, "burst"), (24, "last"), (63, "parity"), (64, "random"))
            for compat in (0, 1)]


@pytest.mark.parametrize("bad,compat,where", RS_CASES, ids=[f"bad{a}-compat{b}-{w}" for a, b, w in RS_CASES])
def test_reed_solomon(po, g, dev, bad, compat, where):
    """the corpus of tests/rxref.py at `bad` bad words per 64-word wavefront (below 24: the wave decoder, from 24 on: the lane decoder), in calls
    of 1000 items down to 1 item; errors 1..16 per word and garbage words.  Output = o_rs_dec_block; with compat = 0 every word with at most 8
    errors is the transmitted payload; the same words give the same output when their wavefront takes the other path."""
    errs = (8, 1, 8, 5, 8, 2) if where == "burst" else tuple(range(1, 17))
    cors = [rxref.rs_corpus(po, n * 8, bad, errors=errs, where=where, garbage_every=9 if bad > 1 else 0, seed=100 * bad + j)
            for j, n in enumerate(RS_CALLS)]
    words = np.concatenate([cr["words"] for cr in cors])
    payload = np.concatenate([cr["payload"] for cr in cors])
    nerr = np.concatenate([cr["nerr"] for cr in cors])
    paths = [rxref.rs_path(b) for cr in cors[:3] for b in cr["bad_per_wave"]]     # the whole wavefronts
    assert set(paths) == {"none" if bad == 0 else "wave" if bad < 24 else "lane"}
    assert [rxref.rs_path(b) for cr in cors[3:] for b in cr["bad_per_wave"]] == [rxref.rs_path(min(bad, 24)), rxref.rs_path(min(bad, 8))]
    rs = po.RS()
    po.lib().o_rs_init(C.byref(rs))
    ref = np.zeros((len(words), 188), np.uint8)
    nf, nc = C.c_int(), C.c_int()
    po.lib().o_rs_dec_block(C.byref(rs), _p(words), _p(ref), C.c_size_t(len(words)), compat, C.byref(nf), C.byref(nc))
    if compat == 0:
        ok = (nerr >= 0) & (nerr <= 8)
        assert (ref[ok] == payload[ok]).all()
    runs = {}
    for entry in ENTRIES:
        b = g.Block("reed_solomon_dec", 2, 8, 0x11d, 255, 239, 8, 51, 8, compat)
        outs, w = [], 0
        for n in RS_CALLS:
            r, cons, _, out = _call(entry, dev, b, n, n, words[w:w + n * 8], n * 8 * 188)
            assert r == cons == n
            outs.append(out.reshape(-1, 188))
            w += n * 8
        b.close()
        got = np.concatenate(outs)
        wrong = np.flatnonzero((got != ref).any(axis=1))
        assert len(wrong) == 0, (entry, wrong[:8], nerr[wrong[:8]])
        if compat == 0:
            assert (got[ok] == payload[ok]).all()
        runs[entry] = got
    assert (runs["host"] == runs["device"]).all()
    # the words of a dense call again, 16 to a wavefront among clean words (and the other way round): the other decoder, the same bytes
    clean = rxref.rs_corpus(po, 64 * 32, 0, seed=7)["words"]
    mix = clean.copy()
    sel = np.arange(512) if bad < 24 else np.flatnonzero(nerr)[:512]
    slots = (np.arange(len(sel)) // 16) * 64 + np.arange(len(sel)) % 16
    if bad < 24:                                              # sparse words packed 48 to a wavefront: the lane decoder
        sel = np.flatnonzero(nerr)[:24 * 32]
        slots = (np.arange(len(sel)) // 48) * 64 + np.arange(len(sel)) % 48
    mix[slots] = words[sel]
    b = g.Block("reed_solomon_dec", 2, 8, 0x11d, 255, 239, 8, 51, 8, compat)
    r, _, _, out = _call("device", dev, b, len(mix) // 8, len(mix) // 8, mix, len(mix) * 188)
    b.close()
    if len(sel):
        assert (out.reshape(-1, 188)[slots] == runs["host"][sel]).all()


# ---------------------------------------------------------------- energy_descramble
def _descr_stream(po, offset, seed, npk=8 * 120):
    rng = np.random.RandomState(seed)
    ts = po.make_ts(npk, seed)
    disp = np.zeros_like(ts)
    po.lib().o_energy_dispersal(_p(ts), _p(disp), C.c_size_t(npk))
    junk = rng.randint(0, 256, (offset, 188)).astype(np.uint8)
    junk[:, 0] = rxref.SYNC
    x = np.concatenate([junk.reshape(-1), disp])
    return x[:len(x) // 1504 * 1504]


def _descr_run(g, dev, entry, x, calls):
    b = g.Block("energy_descramble", 8)
    pos, res = 0, []
    xin = dev.up(x) if entry == "device" else None
    for k in calls:
        avail = (len(x) - pos) // 1504
        if avail < k:
            break
        assert b.forecast(k * 1504) == 4 * k
        if entry == "host":
            out = np.zeros(k * 1504, np.uint8)
            r, cons, _ = b.work(k * 1504, avail, x[pos:], out)
        else:
            o = dev.buf(k * 1504)
            r, cons, _ = b.work_device(k * 1504, avail, xin.data_ptr() + pos, o.data_ptr(), (), dev.s.cuda_stream)
            dev.s.synchronize()
            out = o[:k * 1504].cpu().numpy()
        res.append((cons, r, out[:r]))
        pos += cons * 1504
    b.close()
    return res


def _descr_check(g, dev, x, calls):
    ref, _ = rxref.descramble_calls(x, calls)
    assert len(ref) > 3
    for entry in ENTRIES:
        got = _descr_run(g, dev, entry, x, calls)
        assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in ref], entry
        for i, ((_, _, a), (_, _, b)) in enumerate(zip(got, ref)):
            assert (a == b).all(), (entry, i)
    return ref


@pytest.mark.parametrize("offset", range(16))
def test_energy_descramble_offsets(po, g, dev, offset):
    """the first group starts `offset` packets in; calls of 4, 8, 12 and 64 groups in mixed sizes: per call the restatement's consumed and
    produced counts and bytes, and the transmitted TS"""
    x = _descr_stream(po, offset, 80 + offset)
    calls = [(4, 8, 12, 64)[(i + offset) % 4] for i in range(12)]
    ref = _descr_check(g, dev, x, calls)
    assert all(r[1] > 0 for r in ref)


def test_energy_descramble_lost_and_slipped_sync(po, g, dev):
    """a stretch without NSYNC (two items dropped per call, the search back at offset 0), then a one-packet slip in the middle of the stream (the
    lock moves on from the carried offset)"""
    x = _descr_stream(po, 5, 90, npk=8 * 160)
    x[30 * 1504:36 * 1504:188] = rxref.SYNC
    x = np.concatenate([x[:80 * 1504 + 188 * 6], x[80 * 1504 + 188 * 7:]])
    x = x[:len(x) // 1504 * 1504]
    calls = [4, 8, 4, 12, 4, 4, 8] * 12
    ref = _descr_check(g, dev, x, calls)
    assert any(r[1] == 0 and r[0] == 2 for r in ref)
    assert sum(r[0] for r in ref) > 100
