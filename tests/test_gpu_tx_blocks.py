"""The transmit blocks one at a time (dvbt_<blk>_* of dvbt_txblocks.inc, gr_dvbt_amd.Block) and the TxFlowgraph that chains them.

Each block against the oracle's restatement of its reference block (or a numpy one where the oracle has none), in host and device
entries, whole and split over calls; the chain against the fused modulator (gr_dvbt_amd.Tx): the IFFT input bit-exact, the baseband
within 1e-5 of the peak; and one chain's baseband decoded by the receiver back to the packets.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import txref  # noqa: E402

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    return gr_dvbt_amd


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()


def _work_device(blk, nout, nin, x_bytes, out_nbytes, in_off=0):
    """one work_device call on a copy of x in device memory; returns (produced, consumed, output bytes)"""
    din = _dev(x_bytes)
    dout = torch.zeros(out_nbytes + 64, dtype=torch.uint8, device="cuda")
    r, cons, _ = blk.work_device(nout, nin, din.data_ptr() + in_off, dout.data_ptr())
    torch.cuda.synchronize()
    return r, cons, dout[:out_nbytes].cpu().numpy()


# ---------------------------------------------------------------- energy_dispersal
def _dispersal_ref(po, ts):
    ref = np.zeros_like(ts)
    po.lib().o_energy_dispersal(_p(ts), _p(ref), C.c_size_t(len(ts) // 188))
    return ref


@pytest.mark.parametrize("nblocks", [1, 4])
def test_energy_dispersal_equals_oracle(po, g, nblocks):
    item = 1504 * nblocks
    ts = po.make_ts(8 * nblocks * 5, 11)
    ref = _dispersal_ref(po, ts)
    blk = g.Block("energy_dispersal", nblocks)
    assert blk.forecast(3) == 8 * 189 * nblocks * 3
    garbage = np.arange(37, dtype=np.uint8) | 1                       # no 0x47 in it
    x = np.concatenate([garbage, ts, np.full(200, 0x47, np.uint8)])
    out = np.zeros(5 * item, np.uint8)
    r, cons, _ = blk.work(5, len(x), x, out)
    assert r == 5 and cons == 37 + 5 * item and (out == ref).all()
    r, cons, o = _work_device(blk, 5, len(x), x, 5 * item)
    assert r == 5 and cons == 37 + 5 * item and (o == ref).all()
    blk.close()


def test_energy_dispersal_malformed_sync_and_no_sync(po, g):
    ts = po.make_ts(16, 12)
    ref = _dispersal_ref(po, ts)
    bad = ts.copy()
    bad[188 * 3] = 0x12                                               # a malformed sync byte: written as 0x47 all the same
    bad[188 * 8] = 0x00                                               # and the first of a group: 0xB8
    blk = g.Block("energy_dispersal", 1)
    out = np.zeros(2 * 1504, np.uint8)
    assert blk.work(2, len(bad), bad, out)[:2] == (2, 2 * 1504) and (out == ref).all()
    nosync = np.full(400, 0x11, np.uint8)
    assert blk.work(1, len(nosync), nosync, out)[:2] == (0, 188)
    assert _work_device(blk, 1, len(nosync), nosync, 1504)[:2] == (0, 188)
    blk.close()


# ---------------------------------------------------------------- reed_solomon_enc
def test_reed_solomon_enc_equals_oracle(po, g):
    L = po.lib()
    rs = po.RS()
    L.o_rs_init(C.byref(rs))
    items, blocks = 5, 8
    ts = np.random.RandomState(3).randint(0, 256, (items * blocks, 188)).astype(np.uint8)
    ref = np.zeros((items * blocks, 204), np.uint8)
    for w in range(items * blocks):
        cw = np.zeros(255, np.uint8)
        cw[51:239] = ts[w]
        par = np.zeros(16, np.uint8)
        L.o_rs_encode(C.byref(rs), _p(cw), _p(par))
        ref[w, :188], ref[w, 188:] = ts[w], par
    blk = g.Block("reed_solomon_enc", 2, 8, 0x11d, 255, 239, 8, 51, blocks)
    out = np.zeros_like(ref)
    assert blk.work(items, items, ts, out)[:2] == (items, items) and (out == ref).all()
    r, cons, o = _work_device(blk, items, items, ts, ref.size)
    assert (r, cons) == (items, items) and (o == ref.reshape(-1)).all()
    blk.close()
    with pytest.raises(g.DvbtError):
        g.Block("reed_solomon_enc", 2, 8, 0x11d, 255, 223, 16, 0, 8)


# ---------------------------------------------------------------- convolutional_interleaver
def _fifo_interleave(x, I, M):
    """the reference's FIFOs (convolutional_interleaver_impl.cc:73-82), restated"""
    fifo = [[0] * (M * j) for j in range(I)]
    out = np.zeros_like(x)
    for t in range(len(x)):
        j = t % I
        if M * j == 0:
            out[t] = x[t]
        else:
            fifo[j].insert(0, int(x[t]))
            out[t] = fifo[j].pop()
    return out


def test_convolutional_interleaver_equals_oracle_and_splits(po, g):
    blocks, I, M = 136, 12, 17
    item = I * blocks
    x = np.random.RandomState(5).randint(0, 256, 9 * item).astype(np.uint8)
    ref = np.zeros_like(x)
    po.lib().o_conv_interleave(_p(x), _p(ref), C.c_size_t(len(x)))
    blk = g.Block("convolutional_interleaver", blocks, I, M)
    assert blk.forecast(3 * item) == 3
    out = np.zeros_like(x)
    assert blk.work(9 * item, 9, x, out)[:2] == (9 * item, 9) and (out == ref).all()
    blk.close()
    rng = np.random.RandomState(6)
    blk = g.Block("convolutional_interleaver", blocks, I, M)
    dx, dout = _dev(x), torch.zeros(len(x) + 64, dtype=torch.uint8, device="cuda")
    pos = 0
    while pos < 9:
        n = min(int(rng.randint(1, 4)), 9 - pos)
        r, cons, _ = blk.work_device(n * item, n, dx.data_ptr() + pos * item, dout.data_ptr() + pos * item)
        assert (r, cons) == (n * item, n)
        pos += n
    torch.cuda.synchronize()
    assert (dout[:len(x)].cpu().numpy() == ref).all()
    blk.close()


@pytest.mark.parametrize("blocks,I,M", [(2, 4, 3), (3, 8, 5), (1, 12, 17), (4, 1, 9)])
def test_convolutional_interleaver_other_sizes(g, blocks, I, M):
    item = I * blocks
    x = np.random.RandomState(I * M).randint(0, 256, 40 * item).astype(np.uint8)
    ref = _fifo_interleave(x, I, M)
    blk = g.Block("convolutional_interleaver", blocks, I, M)
    out = np.zeros_like(x)
    pos = 0
    rng = np.random.RandomState(1)
    while pos < 40:
        n = min(int(rng.randint(1, 7)), 40 - pos)
        assert blk.work(n * item, n, x[pos * item:], out[pos * item:])[:2] == (n * item, n)
        pos += n
    assert (out == ref).all()
    blk.close()


# ---------------------------------------------------------------- inner_coder
_PUNCT = {0: "X1Y1", 1: "X1Y1Y2", 2: "X1Y1Y2X3", 3: "X1Y1Y2X3Y4X5", 4: "X1Y1Y2Y3Y4X5Y6X7"}


def _inner_code(x, m, cr):
    """generate_punctured_code (inner_coder_impl.cc:33-121) + packing m bits per byte, restated in numpy"""
    bits = np.unpackbits(x)
    reg = np.concatenate([np.zeros(6, np.uint8), bits])
    n0 = len(bits)
    # x / y of info bit t: G1 = 171, G2 = 133 over bits t, t-1, .., t-6
    w = [reg[6 - d:6 - d + n0] for d in range(7)]
    X = w[0] ^ w[1] ^ w[2] ^ w[3] ^ w[6]
    Y = w[0] ^ w[2] ^ w[3] ^ w[5] ^ w[6]
    pat = _PUNCT[cr]
    k = int(pat[-1])
    per = n0 // k
    cols = [(X if c == "X" else Y)[int(i) - 1::k][:per] for c, i in zip(pat[0::2], pat[1::2])]
    coded = np.stack(cols, axis=1).reshape(-1)
    coded = coded[:len(coded) // m * m].reshape(-1, m)
    return (coded << np.arange(m - 1, -1, -1, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


@pytest.mark.parametrize("const", [0, 1, 2])
@pytest.mark.parametrize("cr", [0, 1, 2, 3, 4])
def test_inner_coder_all_rates(g, const, cr):
    m = (2, 4, 6)[const]
    k, n = (1, 2, 3, 5, 7)[cr], (2, 3, 4, 6, 8)[cr]
    P = 1512
    blk = g.Block("inner_coder", 1, P, const, 0, cr)
    nin4 = 4 * P * k * m // (8 * n)
    assert blk.forecast(8) == 2 * nin4
    x = np.random.RandomState(10 * const + cr).randint(0, 256, 6 * nin4).astype(np.uint8)
    ref = _inner_code(x, m, cr)
    assert len(ref) == 24 * P
    out = np.zeros(24 * P, np.uint8)
    assert blk.work(24, len(x), x, out)[:2] == (24, 6 * nin4) and (out == ref).all()
    blk.close()
    # the same stream split over calls of 4, 8, 12 items, device entry; a call with too little input makes the largest multiple of 4 it can
    blk = g.Block("inner_coder", 1, P, const, 0, cr)
    dx, dout = _dev(x), torch.zeros(24 * P + 64, dtype=torch.uint8, device="cuda")
    rpos = wpos = 0
    for nitems in (4, 8, 12):
        r, cons, _ = blk.work_device(nitems, len(x) - rpos, dx.data_ptr() + rpos, dout.data_ptr() + wpos * P)
        assert (r, cons) == (nitems, nitems // 4 * nin4)
        rpos += cons
        wpos += r
    torch.cuda.synchronize()
    assert (dout[:24 * P].cpu().numpy() == ref).all()
    assert blk.work_device(8, nin4 + 3, dx.data_ptr(), dout.data_ptr())[:2] == (4, nin4)
    blk.close()


def test_inner_coder_refusals_leave_the_stream(g):
    P, cr, const = 6048, 4, 2
    k, n, m = 7, 8, 6
    nin4 = 4 * P * k * m // (8 * n)
    x = np.random.RandomState(2).randint(0, 256, 3 * nin4).astype(np.uint8)
    ref = _inner_code(x, m, cr)
    blk = g.Block("inner_coder", 1, P, const, 0, cr)
    out = np.zeros(12 * P, np.uint8)
    assert blk.work(4, len(x), x, out)[:2] == (4, nin4)
    with pytest.raises(g.DvbtError):
        blk.work(6, len(x) - nin4, x[nin4:], out[4 * P:])            # not a multiple of 4
    assert blk.work(8, len(x) - nin4, x[nin4:], out[4 * P:])[:2] == (8, 2 * nin4)
    assert (out == ref).all()
    blk.close()
    for bad in ((1, 1000, 2, 0, 4), (2, 6048, 2, 0, 4)):
        with pytest.raises(g.DvbtError):
            g.Block("inner_coder", *bad)


# ---------------------------------------------------------------- bit_inner_interleaver
@pytest.mark.parametrize("const,mode", [(0, 0), (1, 1), (2, 0), (2, 1)])
def test_bit_inner_interleaver_equals_oracle(po, g, const, mode):
    c = po.cfg(const, po.C1_2, mode)
    x = np.random.RandomState(4).randint(0, c.csize, (3, c.payload)).astype(np.uint8)
    ref = np.zeros_like(x)
    po.lib().o_bit_interleave(C.byref(c), _p(x), _p(ref), C.c_size_t(x.size))
    blk = g.Block("bit_inner_interleaver", c.payload, const, 0, mode)
    out = np.zeros_like(x)
    assert blk.work(3, 3, x, out)[:2] == (3, 3) and (out == ref).all()
    r, cons, o = _work_device(blk, 3, 3, x, x.size)
    assert (o == ref.reshape(-1)).all()
    de = g.Block("bit_inner_deinterleaver", c.payload, const, 0, mode)
    back = np.zeros_like(x)
    de.work(3, 3, out, back)
    assert (back == x).all()
    blk.close()
    de.close()


def test_bit_inner_interleaver_refuses_hierarchy(g):
    for h in (1, 2, 3):
        with pytest.raises(g.DvbtError):
            g.Block("bit_inner_interleaver", 1512, 2, h, 0)


# ---------------------------------------------------------------- dvbt_map
@pytest.mark.parametrize("const,hier,gain", [(0, 0, 1.0), (1, 0, 1.0), (2, 0, 0.5), (1, 2, 1.0), (1, 3, 2.0), (2, 1, 1.0), (2, 2, 1.0), (2, 3, 0.25)])
def test_map_equals_oracle_points(po, g, const, hier, gain):
    c = po.cfg(const, po.C1_2, po.T2k, hierarchy=hier)
    pts = np.zeros(c.csize, np.complex64)
    po.lib().o_constellation(C.byref(c), C.c_float(gain), _p(pts))
    x = np.random.RandomState(9).randint(0, c.csize, (4, c.payload)).astype(np.uint8)
    blk = g.Block("map", c.payload, const, hier, po.T2k, gain)
    out = np.zeros(x.shape, np.complex64)
    assert blk.work(4, 4, x, out)[:2] == (4, 4)
    assert (out.view(np.uint64) == pts[x].view(np.uint64)).all()
    r, cons, o = _work_device(blk, 4, 4, x, out.nbytes)
    assert (o == out.view(np.uint8).reshape(-1)).all()
    blk.close()
    if hier == 0 and gain == 1.0:
        dm = g.Block("demap", c.payload, const, 0, po.T2k, 1.0)
        lab = np.zeros_like(x)
        dm.work(4, 4, out, lab)
        assert (lab == x).all()
        dm.close()


# ---------------------------------------------------------------- reference_signals
@pytest.mark.parametrize("const,cr,mode,guard,cid_on,cid", [(1, 0, 0, 0, 0, 0), (2, 4, 1, 0, 0, 0), (0, 2, 0, 2, 1, 0x5a)])
def test_reference_signals_equals_fused_carriers(g, const, cr, mode, guard, cid_on, cid):
    d = g.get_dims(const, cr, mode, guard)
    N, P = d.fft_length, d.payload_length
    nsym = 68 * 4 + 9                                                  # a superframe and a few symbols
    npk = -(-nsym * d.info_bits_per_symbol // 1632)
    tx = g.Tx(const, cr, mode, guard=guard, include_cell_id=cid_on, cell_id=cid, max_packets=npk, keep_carriers=True)
    tx.run(_ts(npk))
    car = tx.carriers()[:nsym]
    assert car.shape == (nsym, N)
    cls = lambda s: 4 if s % 68 == 0 else (s % 68) % 4
    # the payload carriers of every symbol, in carrier order, from the fused modulator's own frames: the input of reference_signals
    zl = d.zeros_on_left
    mask = {}
    pay = np.zeros((nsym, P), np.complex64)
    blk0 = g.Block("reference_signals", 8, P, N, const, 0, cr, cr, guard, mode, cid_on, cid)
    zero = np.zeros((4 * 5, P), np.complex64)
    o0 = np.zeros((4 * 5, N), np.complex64)
    blk0.work(20, 20, zero, o0)                                        # symbols 0..19: pilots and TPS alone
    blk0.close()
    for s in range(nsym):
        c = cls(s)
        if c not in mask:
            ref_sym = {4: 0, 1: 1, 2: 2, 3: 3, 0: 4}[c]
            mask[c] = np.flatnonzero((o0[ref_sym] == 0))
            mask[c] = mask[c][(mask[c] >= zl) & (mask[c] < zl + d.Kmax + 1)]
            assert len(mask[c]) == P
        pay[s] = car[s, mask[c]]
    blk = g.Block("reference_signals", 8, P, N, const, 0, cr, cr, guard, mode, cid_on, cid)
    out = np.zeros((nsym, N), np.complex64)
    rng = np.random.RandomState(2)
    pos = 0
    host = True
    while pos < nsym:
        n = min(int(rng.randint(1, 60)), nsym - pos)
        if host:
            assert blk.work(n, n, pay[pos:], out[pos:])[:2] == (n, n)
        else:
            r, cons, o = _work_device(blk, n, n, pay[pos:pos + n], n * N * 8)
            assert (r, cons) == (n, n)
            out[pos:pos + n] = o.view(np.complex64).reshape(n, N)
        host = not host
        pos += n
    assert (out.view(np.uint64) == car.view(np.uint64)).all()
    blk.close()


def _ts(npk, seed=7):
    ts = np.random.RandomState(seed).randint(0, 256, (npk, 188)).astype(np.uint8)
    ts[:, 0] = 0x47
    return ts.reshape(-1)


# ---------------------------------------------------------------- the whole chain
@pytest.mark.parametrize("const,cr,mode", [(1, 0, 0), (2, 4, 1), (0, 2, 0)])
@pytest.mark.parametrize("fg_mode", ["host", "device"])
def test_tx_flowgraph_equals_fused_modulator(g, const, cr, mode, fg_mode):
    from gr_dvbt_amd.flowgraph import TxFlowgraph
    d = g.get_dims(const, cr, mode)
    npk = -(-(68 * 4 + 20) * d.info_bits_per_symbol // 1632)
    npk = -(-npk // 32) * 32
    ts = _ts(npk, 3)
    tx = g.Tx(const, cr, mode, max_packets=npk, keep_carriers=True)
    iq_ref = tx.run(ts)
    car_ref = tx.carriers()
    fg = TxFlowgraph(const, cr, mode, mode=fg_mode, call_items=np.random.default_rng(const * 10 + cr))
    bb, car = fg.run(ts)
    fg.close()
    n = car.shape[0]
    assert n >= 68 * 4, n                                              # a superframe at least went through
    assert (car.view(np.uint64) == car_ref[:n].view(np.uint64)).all()
    ref = iq_ref[:len(bb)]
    assert len(bb) == n * (d.fft_length + d.cp_length)
    assert np.abs(bb - ref).max() <= 1e-5 * np.abs(iq_ref).max()


def test_tx_flowgraph_loopback_through_rx(g):
    from gr_dvbt_amd.flowgraph import TxFlowgraph
    const, cr, mode = 1, 0, 0
    d = g.get_dims(const, cr, mode)
    ibits = d.info_bits_per_symbol
    npk = 2 * 272 * ibits // 1632 + 64
    ts = _ts(npk, 5)
    fg = TxFlowgraph(const, cr, mode, mode="device", call_items=6)
    body, _ = fg.run(ts)
    fg.close()
    iq = np.concatenate([np.zeros(1000, np.complex64), body, np.zeros(3 * d.fft_length, np.complex64)])
    rx = g.Rx(const, cr, mode, max_samples=len(iq), taps=True)
    rep = rx.run(iq)
    got_ts = rx.tap(g.TAP_TS)
    p0 = rep.first_out_symbol * ibits // 8 // 204 + rep.ts_first_packet - 11      # as test_gpu_tx: RS word w is the packet sent 11 words earlier
    n = len(got_ts) // 188
    assert n > 100 and p0 >= 0 and p0 + n <= npk
    assert (got_ts.reshape(-1, 188) == ts.reshape(-1, 188)[p0:p0 + n]).all()


# ---------------------------------------------------------------- errors leave the stream intact
def test_refused_calls_leave_state(g):
    # convolutional_interleaver: a count that is not a multiple of I * blocks is refused; the stream goes on
    blocks, I, M = 2, 4, 3
    item = I * blocks
    x = np.random.RandomState(8).randint(0, 256, 12 * item).astype(np.uint8)
    ref = _fifo_interleave(x, I, M)
    blk = g.Block("convolutional_interleaver", blocks, I, M)
    out = np.zeros_like(x)
    assert blk.work(5 * item, 5, x, out)[0] == 5 * item
    with pytest.raises(g.DvbtError):
        blk.work(5 * item + 1, 7, x[5 * item:], out[5 * item:])
    assert blk.work(7 * item, 7, x[5 * item:], out[5 * item:])[0] == 7 * item
    assert (out == ref).all()
    blk.close()
    # reference_signals: a misaligned device output is refused; symbol_index does not move
    d = g.get_dims(1, 0, 0)
    N, P = d.fft_length, d.payload_length
    a = g.Block("reference_signals", 8, P, N, 1, 0, 0, 0, 0, 0, 0, 0)
    bref = g.Block("reference_signals", 8, P, N, 1, 0, 0, 0, 0, 0, 0, 0)
    pay = (np.random.RandomState(3).randn(6, P) + 0j).astype(np.complex64)
    o1, o2 = np.zeros((6, N), np.complex64), np.zeros((6, N), np.complex64)
    a.work(2, 2, pay, o1)
    din = _dev(pay[2:])
    dout = torch.zeros(4 * N * 8 + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(g.DvbtError):
        a.work_device(4, 4, din.data_ptr(), dout.data_ptr() + 4)
    a.work(4, 4, pay[2:], o1[2:])
    bref.work(6, 6, pay, o2)
    assert (o1 == o2).all()
    a.close()
    bref.close()


# ================================================================ the block entries at the sizes the ABI accepts
def _rs_ref(po, ts):
    L = po.lib()
    rs = po.RS()
    L.o_rs_init(C.byref(rs))
    ref = np.zeros((len(ts), 204), np.uint8)
    cw = np.zeros(255, np.uint8)
    par = np.zeros(16, np.uint8)
    for w in range(len(ts)):
        cw[51:239] = ts[w]
        L.o_rs_encode(C.byref(rs), _p(cw), _p(par))
        ref[w, :188], ref[w, 188:] = ts[w], par
    return ref


@pytest.mark.parametrize("npk", [1, 127, 128, 129, 255, 256, 1000])
def test_reed_solomon_enc_packet_counts(po, g, npk):
    """one, part of, exactly and more than one 128-lane workgroup of txb_rs_enc_kernel, with and without a tail workgroup"""
    ts = np.random.RandomState(npk).randint(0, 256, (npk, 188)).astype(np.uint8)
    ref = _rs_ref(po, ts)
    blocks = 8 if npk % 8 == 0 else 1
    items = npk // blocks
    blk = g.Block("reed_solomon_enc", 2, 8, 0x11d, 255, 239, 8, 51, blocks)
    out = np.zeros_like(ref)
    assert blk.work(items, items, ts, out)[:2] == (items, items)
    assert (out == ref).all()
    r, cons, o = _work_device(blk, items, items, ts, ref.size)
    assert (r, cons) == (items, items) and (o == ref.reshape(-1)).all()
    blk.close()


@pytest.mark.parametrize("nblocks", [2, 3, 8, 17, 4096])
def test_energy_dispersal_sizes_prefixes_and_splits(po, g, nblocks):
    """garbage of 0, 1, 187 and 188 bytes (no 0x47) in front of the first sync byte; the stream over calls of 1 or 2 items, host and device
    entries alternating, driven as a scheduler would: every call gets what the previous ones did not consume"""
    item = 1504 * nblocks
    nitems = 1 if nblocks == 4096 else 4
    ts = po.make_ts(8 * nblocks * nitems, 30 + nblocks)
    ref = _dispersal_ref(po, ts)
    rng = np.random.RandomState(nblocks)
    for prefix in (0, 1, 187, 188):
        garbage = rng.randint(0, 256, prefix).astype(np.uint8)
        garbage[garbage == 0x47] = 0x48
        x = np.concatenate([garbage, ts])
        blk = g.Block("energy_dispersal", nblocks)
        out = np.zeros(nitems * item, np.uint8)
        pos = done = calls = 0
        while done < nitems:
            n = min(int(rng.randint(1, 3)), nitems - done)
            if calls % 2 == 0:
                r, cons, _ = blk.work(n, len(x) - pos, x[pos:], out[done * item:])
            else:
                r, cons, o = _work_device(blk, n, len(x) - pos, x[pos:], n * item)
                out[done * item:(done + r) * item] = o[:r * item]
            assert 0 <= r <= n
            pos += cons
            done += r
            calls += 1
            assert calls < 3 * nitems + 4, "the block stopped consuming"
        assert pos == len(x), (prefix, pos)
        assert (out == ref).all(), prefix
        blk.close()


_RATE_KN = {0: (1, 2), 1: (2, 3), 2: (3, 4), 3: (5, 6), 4: (7, 8)}


@pytest.mark.skipif(torch is None, reason="needs torch")
@pytest.mark.parametrize("noutput", [6048, 3 * 1512, 64 * 1512])
@pytest.mark.parametrize("const", [0, 1, 2])
@pytest.mark.parametrize("cr", [0, 1, 2, 3, 4])
def test_inner_coder_output_sizes(g, noutput, const, cr):
    m = (2, 4, 6)[const]
    k, n = _RATE_KN[cr]
    nin4 = 4 * noutput * k * m // (8 * n)
    assert nin4 * 8 * n == 4 * noutput * k * m
    calls = (4, 8) if noutput > 6048 else (4, 8, 4, 12)
    total = sum(calls)
    x = np.random.RandomState(1000 * const + 10 * cr + noutput % 97).randint(0, 256, total // 4 * nin4).astype(np.uint8)
    ref = _inner_code(x, m, cr)
    assert len(ref) == total * noutput
    blk = g.Block("inner_coder", 1, noutput, const, 0, cr)
    assert blk.forecast(4) == nin4
    out = np.zeros(total * noutput, np.uint8)
    dx, dout = _dev(x), torch.zeros(total * noutput + 64, dtype=torch.uint8, device="cuda")
    rpos = wpos = 0
    for i, nitems in enumerate(calls):
        if i % 2 == 0:
            r, cons, _ = blk.work(nitems, len(x) - rpos, x[rpos:], out[wpos * noutput:])
        else:
            r, cons, _ = blk.work_device(nitems, len(x) - rpos, dx.data_ptr() + rpos, dout.data_ptr() + wpos * noutput)
            torch.cuda.synchronize()
            out[wpos * noutput:(wpos + r) * noutput] = dout[wpos * noutput:(wpos + r) * noutput].cpu().numpy()
        assert (r, cons) == (nitems, nitems // 4 * nin4)
        rpos += cons
        wpos += r
    assert rpos == len(x)
    assert (out == ref).all()
    blk.close()


@pytest.mark.parametrize("nsize", [252, 504, 1512, 6048, 49392])
@pytest.mark.parametrize("const", [0, 1, 2])
def test_bit_inner_interleaver_sizes(po, g, nsize, const):
    c = po.cfg(const, po.C1_2, po.T2k)
    items = 2 if nsize > 6048 else 3
    x = np.random.RandomState(nsize + const).randint(0, c.csize, (items, nsize)).astype(np.uint8)
    ref = np.zeros_like(x)
    po.lib().o_bit_interleave(C.byref(c), _p(x), _p(ref), C.c_size_t(x.size))   # whole 126-word blocks, any number of them
    blk = g.Block("bit_inner_interleaver", nsize, const, 0, po.T2k)
    out = np.zeros_like(x)
    assert blk.work(items, items, x, out)[:2] == (items, items) and (out == ref).all()
    r, cons, o = _work_device(blk, items, items, x, x.size)
    assert (r, cons) == (items, items) and (o == ref.reshape(-1)).all()
    blk.close()


@pytest.mark.parametrize("const", [0, 1, 2])
@pytest.mark.parametrize("hier", [0, 1, 2, 3])
def test_map_every_label_gain_and_size(po, g, const, hier):
    c = po.cfg(const, po.C1_2, po.T2k, hierarchy=hier)
    for gain in (1.0, 0.5, float(np.pi / 7)):
        pts = np.zeros(c.csize, np.complex64)
        po.lib().o_constellation(C.byref(c), C.c_float(gain), _p(pts))
        for nsize in (2, c.payload):
            rng = np.random.RandomState(nsize + const)
            nl = max(64, 3 * nsize)
            lab = rng.randint(0, 256, nl).astype(np.uint8)
            lab[:64] = np.arange(64)
            lab &= c.csize - 1                                            # labels of the constellation (the reference indexes its table with them)
            items = nl // nsize
            lab = lab[:items * nsize].reshape(items, nsize)
            blk = g.Block("map", nsize, const, hier, po.T2k, gain)
            out = np.zeros(lab.shape, np.complex64)
            assert blk.work(items, items, lab, out)[:2] == (items, items)
            assert out.view(np.uint64).tobytes() == pts[lab].view(np.uint64).tobytes(), (gain, nsize)
            r, cons, o = _work_device(blk, items, items, lab, out.nbytes)
            assert (r, cons) == (items, items) and o.tobytes() == out.tobytes()
            blk.close()


# (const, hier, code rate HP, code rate LP, guard, mode, include_cell_id, cell_id): every value of each parameter at least once, LP != HP three times
REFSIG = [(0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 3, 1, 1, 1, 0x12), (2, 2, 2, 2, 2, 0, 1, 0xff), (2, 3, 3, 0, 3, 1, 0, 0x5a), (1, 0, 4, 4, 1, 0, 0, 0),
          (0, 2, 4, 1, 3, 0, 1, 0x81)]


@pytest.mark.parametrize("const,hier,cr,cr_lp,guard,mode,cid_on,cid", REFSIG)
def test_reference_signals_covering_set(po, g, const, hier, cr, cr_lp, guard, mode, cid_on, cid):
    """the fused modulator's frames (TPS with LP = HP) on every carrier but the TPS ones, and the whole frame where LP = HP; the TPS word decoded
    from the carriers of every frame: the fields at the bit positions of ETSI EN 300 744 4.6.2 and the BCH(67,53) parity"""
    d = g.get_dims(const, cr, mode, guard, hier)
    N, P, zl = d.fft_length, d.payload_length, d.zeros_on_left
    nsym = 68 * 4 + 9
    npk = -(-nsym * d.info_bits_per_symbol // 1632)
    tx = g.Tx(const, cr, mode, guard=guard, hierarchy=hier, include_cell_id=cid_on, cell_id=cid, max_packets=npk, keep_carriers=True)
    tx.run(_ts(npk, 13))
    car = tx.carriers()[:nsym]
    tx.close()
    assert car.shape == (nsym, N)
    args = (8, P, N, const, hier, cr, cr_lp, guard, mode, cid_on, cid)
    blk0 = g.Block("reference_signals", *args)
    o0 = np.zeros((5, N), np.complex64)
    blk0.work(5, 5, np.zeros((5, P), np.complex64), o0)                 # symbols 0..4: pilots and TPS alone, one of every class
    blk0.close()
    cls = lambda s: 4 if s % 68 == 0 else (s % 68) % 4
    mask = {}
    for s in range(5):
        m_ = np.flatnonzero(o0[s] == 0)
        mask[cls(s)] = m_[(m_ >= zl) & (m_ < zl + d.Kmax + 1)]
        assert len(mask[cls(s)]) == P
    pay = np.stack([car[s, mask[cls(s)]] for s in range(nsym)])
    blk = g.Block("reference_signals", *args)
    out = np.zeros((nsym, N), np.complex64)
    rng = np.random.RandomState(mode + 2 * guard)
    pos, host = 0, True
    while pos < nsym:
        n = min(int(rng.randint(1, 90)), nsym - pos)
        if host:
            assert blk.work(n, n, pay[pos:], out[pos:])[:2] == (n, n)
        else:
            r, cons, o = _work_device(blk, n, n, pay[pos:pos + n], n * N * 8)
            assert (r, cons) == (n, n)
            out[pos:pos + n] = o.view(np.complex64).reshape(n, N)
        host = not host
        pos += n
    blk.close()
    c = po.cfg(const, cr, mode, guard=guard, hierarchy=hier, include_cell_id=cid_on, cell_id=cid)
    tcar, wk = txref.tps_carriers(po, c)
    other = np.ones(N, bool)
    other[zl + tcar] = False
    assert out[:, other].view(np.uint64).tobytes() == car[:, other].view(np.uint64).tobytes()
    if cr_lp == cr:
        assert out.view(np.uint64).tobytes() == car.view(np.uint64).tobytes()
    F = txref.tps_field
    for f in range(4):
        t = txref.decode_tps(out[68 * f:68 * (f + 1)], zl, tcar, wk)
        assert t[0] == 0                                                  # the first symbol holds the DBPSK initialisation 2 (1/2 - w_k)
        assert F(t, 1, 16) == (0x35ee if f % 2 == 0 else 0xca11)           # 4.6.2.2: the sync word in frames 1 and 3, inverted in 2 and 4
        assert F(t, 17, 22) == (0b011111 if cid_on else 0b010111)          # 4.6.2.3: 31 or 23 TPS bits in use
        assert F(t, 23, 24) == f                                           # 4.6.2.4
        assert F(t, 25, 26) == const and F(t, 27, 29) == hier              # 4.6.2.5, 4.6.2.6
        assert F(t, 30, 32) == cr and F(t, 33, 35) == cr_lp                # 4.6.2.7
        assert F(t, 36, 37) == guard and F(t, 38, 39) == mode              # 4.6.2.8, 4.6.2.9
        # 4.6.2.10 sends the cell id's high byte in frames 1 and 3; the reference writes its low byte into every frame
        # (format_tps_data, set_tps_bits(47, 40, cell_id)), and so does the library
        assert F(t, 40, 47) == cid & 0xff and F(t, 48, 53) == 0
        assert txref.bch_remainder(t[1:]) == 0                             # 4.6.3


@pytest.mark.parametrize("const,cr,mode,guard,cid_on,cid", [(0, 1, 1, 0, 0, 0), (1, 3, 1, 1, 0, 0), (2, 2, 0, 3, 0, 0), (1, 1, 0, 2, 1, 0x33)])
@pytest.mark.parametrize("fg_mode", ["host", "device"])
def test_tx_flowgraph_more_configurations(g, const, cr, mode, guard, cid_on, cid, fg_mode):
    """test_tx_flowgraph_equals_fused_modulator at 8k QPSK, 8k QAM16, GI 1/4 and with a cell id"""
    from gr_dvbt_amd.flowgraph import TxFlowgraph
    d = g.get_dims(const, cr, mode, guard)
    npk = -(-(68 * 4 + 20) * d.info_bits_per_symbol // 1632)
    npk = -(-npk // 32) * 32
    ts = _ts(npk, 4)
    tx = g.Tx(const, cr, mode, guard=guard, include_cell_id=cid_on, cell_id=cid, max_packets=npk, keep_carriers=True)
    iq_ref = tx.run(ts)
    car_ref = tx.carriers()
    tx.close()
    fg = TxFlowgraph(const, cr, mode, guard=guard, mode=fg_mode, call_items=np.random.default_rng(const * 10 + cr + guard),
                     include_cell_id=cid_on, cell_id=cid)
    bb, car = fg.run(ts)
    fg.close()
    n = car.shape[0]
    assert n >= 68 * 4, n
    assert (car.view(np.uint64) == car_ref[:n].view(np.uint64)).all()
    assert len(bb) == n * (d.fft_length + d.cp_length)
    assert np.abs(bb - iq_ref[:len(bb)]).max() <= 1e-5 * np.abs(iq_ref).max()
