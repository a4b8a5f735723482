"""GPU modulator (dvbt_tx_*, gr_dvbt_amd.Tx) against the oracle's generator o_tx_generate_from.

The frequency-domain frames (the IFFT input: payload, pilots, TPS) must be bit-exact; the baseband is compared within 1e-5 of the
oracle's peak sample (the bound of the FFT tap, test_gpu_blocks.test_fft_block).  A stream split over calls of any size must give
what one call gives, and the GPU receiver must decode the GPU transmitter's signal to the transmitted packets.
"""
import numpy as np
import pytest

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


def _ref(po, c, ts, scale, first_packet=0):
    iq, freq = po.tx(c, ts, scale=scale, want_freq=True, packet0=first_packet)
    return iq, freq


def _close(a, b):
    assert a.shape == b.shape and len(b) > 0
    assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max()


# (constellation, code rate, mode, guard, hierarchy, include_cell_id, cell_id, first_packet)
CONFIGS = [
    (1, 0, 0, 0, 0, 0, 0, 0),          # BASELINE: 2k QAM16 1/2
    (2, 4, 1, 0, 0, 0, 0, 0),          # BASELINE: 8k QAM64 7/8
    (0, 4, 1, 1, 0, 0, 0, 0),          # BASELINE: 8k QPSK 7/8, GI 1/16
    (0, 2, 0, 2, 0, 0, 0, 13),         # 2k QPSK 3/4 (283.5 bytes per symbol), GI 1/8, dispersal phase 13
    (1, 3, 1, 3, 0, 1, 0x5a, 0),       # 8k QAM16 5/6, GI 1/4, cell id in the TPS
    (2, 1, 0, 3, 2, 0, 0, 5),          # 2k QAM64 2/3, hierarchical alpha = 2
]


@pytest.mark.parametrize("const,cr,mode,guard,hier,cid_on,cid,fp", CONFIGS)
def test_carriers_exact_and_baseband(po, g, const, cr, mode, guard, hier, cid_on, cid, fp):
    c = po.cfg(const, cr, mode, guard=guard, hierarchy=hier, include_cell_id=cid_on, cell_id=cid)
    npk = 2 * po.packets_per_superframe(c) + 37
    ts = po.make_ts(npk, 7)
    scale = 0.0022097087
    iq_ref, freq_ref = _ref(po, c, ts, scale, fp)
    assert len(freq_ref) > 2 * 4 * 68 - 1                            # every frame index and every symbol_index mod 4, twice
    tx = g.Tx(const, cr, mode, guard=guard, hierarchy=hier, include_cell_id=cid_on, cell_id=cid, scale=scale, max_packets=npk,
              first_packet=fp, keep_carriers=True)
    assert tx.samples_for(npk) == len(iq_ref)
    iq = tx.run(ts)
    car = tx.carriers()
    assert car.shape == freq_ref.shape and (car == freq_ref).all()
    _close(iq, iq_ref)
    tx.close()


@pytest.mark.parametrize("const,cr,mode", [(0, 2, 0), (2, 4, 1)])
def test_streaming_equals_one_call(po, g, const, cr, mode):
    c = po.cfg(const, cr, mode)
    npk = 3 * po.packets_per_superframe(c)
    ts = po.make_ts(npk, 3)
    scale = po.tx_scale(c)
    iq_ref, freq_ref = _ref(po, c, ts, scale)
    splits = [1, 7, 1000, 0, npk - 1008]
    tx = g.Tx(const, cr, mode, scale=scale, max_packets=npk, keep_carriers=True)
    outs, cars, p = [], [], 0
    for n in splits:
        want = tx.samples_for(n)
        o = tx.run(ts[p * 188:(p + n) * 188])
        assert len(o) == want
        outs.append(o)
        cars.append(tx.carriers())
        p += n
    assert len(outs[0]) == 0                                       # one packet completes no symbol
    assert (np.concatenate(cars) == freq_ref).all()
    _close(np.concatenate(outs), iq_ref)
    # reset: the same handle starts the stream again
    tx.reset()
    _close(tx.run(ts), iq_ref)
    assert (tx.carriers() == freq_ref).all()
    tx.close()


@pytest.mark.parametrize("const,cr,mode,nsf", [(2, 4, 1, 2), (1, 0, 0, 3)])
def test_loopback_through_the_gpu_receiver(po, g, const, cr, mode, nsf):
    c = po.cfg(const, cr, mode)
    ibits = c.payload * c.m * c.k // c.n
    npk = (272 * ibits * nsf) // (204 * 8)
    ts = po.make_ts(npk, 11)
    lead, tail = 1000, 3 * c.N
    scale = po.tx_scale(c)
    tx = g.Tx(const, cr, mode, scale=scale, max_packets=npk)
    body = tx.run(ts)
    tx.close()
    iq = np.concatenate([np.zeros(lead, np.complex64), body, np.zeros(tail, np.complex64)])
    rx = g.Rx(const, cr, mode, max_samples=len(iq), taps=True)
    rep = rx.run(iq)
    got_ts = rx.tap(g.TAP_TS)
    # the TS tap starts ts_first_packet RS words after the superframe start; RS word w is the packet sent 11 words earlier
    p0 = rep.first_out_symbol * ibits // 8 // 204 + rep.ts_first_packet - 11
    n = len(got_ts) // 188
    assert n > 0 and p0 >= 0 and p0 + n <= npk
    assert (got_ts.reshape(-1, 188) == ts.reshape(-1, 188)[p0:p0 + n]).all()
    # the oracle's receiver on the oracle's transmitter: the same decisions from the demapper on
    o = po.rx(c, po.tx(c, ts, lead_in=lead, tail=tail), want=("demap", "symdeint", "bitdeint", "vit", "deint", "rs", "ts"))
    assert rep.first_out_symbol == o["first_out_symbol"]
    for name, tap in (("demap", g.TAP_DEMAP), ("symdeint", g.TAP_SYMDEINT), ("bitdeint", g.TAP_BITDEINT), ("vit", g.TAP_VITERBI),
                      ("deint", g.TAP_DEINT), ("rs", g.TAP_RS), ("ts", g.TAP_TS)):
        a, b = rx.tap(tap), o[name]
        assert a.size == b.size > 0, name
        assert (a.reshape(-1) == b.reshape(-1)).all(), name
    rx.close()


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_device_entry_on_streams(po, g):
    c = po.cfg(1, 0, 0)
    npk = po.packets_per_superframe(c) + 91
    ts = po.make_ts(npk, 5)
    ts2 = po.make_ts(npk, 6)
    scale = 0.0022097087
    ref1 = g.Tx(1, 0, 0, scale=scale, max_packets=npk).run(ts)
    ref2 = g.Tx(1, 0, 0, scale=scale, max_packets=npk).run(ts2)
    dev = torch.device("cuda:0")
    dts, dts2 = torch.from_numpy(ts).to(dev), torch.from_numpy(ts2).to(dev)
    cap = len(ref1) + 4096
    out1 = torch.zeros(cap * 2, dtype=torch.float32, device=dev)
    out2 = torch.zeros(cap * 2, dtype=torch.float32, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = g.Tx(1, 0, 0, scale=scale, max_packets=npk)
    b = g.Tx(1, 0, 0, scale=scale, max_packets=npk)
    torch.cuda.synchronize()
    # two handles interleaved on two streams, each in three calls; handle a changes streams between its calls
    cuts = [0, 300, 301, npk]
    na = nb = 0
    for i in range(3):
        lo, hi = cuts[i], cuts[i + 1]
        sa = s1 if i != 1 else s2
        na += a.run_device(dts.data_ptr() + lo * 188, hi - lo, out1.data_ptr() + na * 8, cap - na, stream=sa.cuda_stream)
        nb += b.run_device(dts2.data_ptr() + lo * 188, hi - lo, out2.data_ptr() + nb * 8, cap - nb, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    got1 = out1.cpu().numpy().view(np.complex64)[:na]
    got2 = out2.cpu().numpy().view(np.complex64)[:nb]
    assert na == len(ref1) and nb == len(ref2)
    assert got1.tobytes() == ref1.tobytes() and got2.tobytes() == ref2.tobytes()
    a.close(); b.close()


def test_inverse_fft_block(po, g):
    import ctypes as C
    rng = np.random.RandomState(4)
    for N in (2048, 8192):
        x = (rng.randn(5, N) + 1j * rng.randn(5, N)).astype(np.complex64)
        ref = np.zeros_like(x)
        for i in range(5):
            po.lib().o_ifft_shift(N, x[i].ctypes.data_as(C.c_void_p), ref[i].ctypes.data_as(C.c_void_p))
        b = g.Block("fft", N, 0, 1)
        out = np.zeros_like(x)
        r, cons, _ = b.work(5, 5, x, out)
        assert r == 5 and cons == 5
        peak = np.abs(ref).max()
        assert np.abs(out - ref).max() <= 1e-5 * peak
        np_ref = np.fft.ifft(np.fft.ifftshift(x.astype(np.complex128), axes=1), axis=1) * N
        assert np.abs(out - np_ref).max() <= 1e-5 * peak
        fwd = g.Block("fft", N, 1, 1)
        back = np.zeros_like(x)
        fwd.work(5, 5, out, back)                                  # FFT(IFFT(x)) = N x (both shifted)
        assert np.abs(back - N * x).max() <= 1e-5 * np.abs(N * x).max()
        b.close(); fwd.close()
    with pytest.raises(g.DvbtError):
        g.Block("fft", 2048, 0, 0)
    with pytest.raises(g.DvbtError):
        g.Block("fft", 1000, 0, 1)


def test_errors_leave_the_stream_intact(po, g):
    import ctypes as C
    c = po.cfg(0, 2, 0)
    npk = po.packets_per_superframe(c) + 11
    ts = po.make_ts(npk, 8)
    scale = 0.0022097087
    iq_ref, freq_ref = _ref(po, c, ts, scale)
    for bad in (dict(scale=0.0), dict(scale=-1.0), dict(max_packets=0), dict(first_packet=-1), dict(guard=4), dict(mode=2)):
        kw = dict(const=0, cr=2, mode=0, guard=0, scale=scale, max_packets=100, first_packet=0)
        kw.update(bad)
        with pytest.raises(g.DvbtError):
            g.Tx(kw["const"], kw["cr"], kw["mode"], guard=kw["guard"], scale=kw["scale"], max_packets=kw["max_packets"], first_packet=kw["first_packet"])
    with pytest.raises(g.DvbtError):
        g.Tx(5, 2, 0)
    tx = g.Tx(0, 2, 0, scale=scale, max_packets=600, keep_carriers=True)
    first = tx.run(ts[:100 * 188])
    L = g.lib()
    # too many packets for the handle: refused, state unchanged
    big = np.zeros(601 * 188, np.uint8)
    out = np.zeros(tx.samples_for(600) + 10 * c.N, np.complex64)
    n = C.c_size_t()
    assert L.dvbt_tx_run(tx.h, big.ctypes.data_as(C.c_void_p), 601, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)) == -4
    # an output buffer one sample short: refused, state unchanged
    need = tx.samples_for(200)
    assert need > 0
    assert L.dvbt_tx_run(tx.h, ts[100 * 188:].ctypes.data_as(C.c_void_p), 200, out.ctypes.data_as(C.c_void_p), need - 1, C.byref(n)) == -4
    assert L.dvbt_tx_run_device(tx.h, None, 200, None, need - 1, None, C.byref(n)) == -4
    assert L.dvbt_tx_run_device(tx.h, None, 200, None, need, None, C.byref(n)) == -1      # null buffers
    assert tx.samples_for(200) == need
    rest = tx.run(ts[100 * 188:])
    _close(np.concatenate([first, rest]), iq_ref)
    assert (tx.carriers() == freq_ref[-len(tx.carriers()):]).all()
    tx.close()
