"""The drop-in path: the ten receive blocks driven one general_work-sized call at a time through the per-block C ABI
(gr_dvbt_amd/flowgraph.py), with host buffers (dvbt_<blk>_work) and with device buffers (dvbt_<blk>_work_device).  The TS
must be the oracle's, whatever the call size."""
import numpy as np
import pytest

import gr_dvbt_amd as g
from gr_dvbt_amd.flowgraph import RxFlowgraph

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("const,cr,mode_t,nsf", [(g.QAM16, g.C1_2, g.T2k, 3), (g.QAM64, g.C7_8, g.T8k, 2)])
@pytest.mark.parametrize("mode,call_symbols", [("host", 4), ("device", 1), ("device", 4), ("device", 33)])
def test_block_by_block_equals_the_oracle(po, const, cr, mode_t, nsf, mode, call_symbols):
    c = po.cfg(const, cr, mode_t)
    iq = po.stream_slice(c, nsf, 9)
    ref = po.rx(c, iq, want=("ts",))["ts"]
    fg = RxFlowgraph(const, cr, mode_t, len(iq), mode=mode, call_symbols=call_symbols)
    ts = fg.run(iq)
    calls = [st.calls for st in fg.stages]
    fg.close()
    assert min(calls) > 0
    # the block-by-block chain stops a few items earlier or later than the whole-segment chain depending on where the calls' windows end
    # (the scheduler's leftovers); what it delivers must be the oracle's stream from its first byte on
    n = min(len(ts), len(ref))
    assert n > 0.9 * len(ref) and abs(len(ts) - len(ref)) <= 64 * 1504
    assert (ts[:n] == ref[:n]).all()


@pytest.mark.parametrize("const,cr,mode_t,nsf,call_symbols", [(g.QAM16, g.C1_2, g.T2k, 3, 16), (g.QAM64, g.C7_8, g.T8k, 3, 64)])
def test_thread_per_block_scheduler_equals_the_oracle(po, const, cr, mode_t, nsf, call_symbols):
    """the ten blocks under a thread-per-block scheduler (what GNU Radio's is): every block's general_work in its own thread, calls of whatever size its input
    allows at that moment, host buffers.  The TS must be the oracle's whatever the interleaving of the calls was."""
    c = po.cfg(const, cr, mode_t)
    iq = po.stream_slice(c, nsf, 9)
    ref = po.rx(c, iq, want=("ts",))["ts"]
    for _ in range(2):                                                     # two runs: two different interleavings
        fg = RxFlowgraph(const, cr, mode_t, len(iq), mode="host", call_symbols=call_symbols)
        ts = fg.run_threaded(iq)
        calls = [st.calls for st in fg.stages]
        fg.close()
        assert min(calls) > 0
        n = min(len(ts), len(ref))
        assert n > 0.9 * len(ref) and abs(len(ts) - len(ref)) <= 64 * 1504
        assert (ts[:n] == ref[:n]).all()


@pytest.mark.parametrize("threads", [1, 0], ids=["a thread per block", "one thread"])
def test_cpp_thread_per_block_driver_equals_the_oracle(po, tmp_path, threads):
    """gr_dvbt_amd/host/rx_blocks_bench: the ten blocks over dvbt_<blk>_work (host buffers) under a thread-per-block scheduler written in C++ (the form the
    drop-in path's throughput is measured in: no interpreter between the calls).  The TS file must be the oracle's."""
    import subprocess, json
    from conftest import host_example
    exe = host_example("rx_blocks_bench")
    const, cr, mode_t = g.QAM64, g.C7_8, g.T8k
    c = po.cfg(const, cr, mode_t)
    iq = po.stream_slice(c, 3, 9)
    ref = po.rx(c, iq, want=("ts",))["ts"]
    fin, fout = tmp_path / "bb.cf32", tmp_path / "out.ts"
    iq.tofile(fin)
    out = subprocess.check_output([exe, "8k", "qam64", "7/8", str(fin), str(fout), "64", str(threads)], text=True)
    info = json.loads(out.strip().splitlines()[-1])
    ts = np.fromfile(fout, np.uint8)
    n = min(len(ts), len(ref))
    assert info["samples"] == len(iq) and n > 0.9 * len(ref) and abs(len(ts) - len(ref)) <= 64 * 1504
    assert (ts[:n] == ref[:n]).all()


def test_registered_host_buffers(po, tmp_path):
    """dvbt_host_register: the flowgraph's buffers page-locked once; the host-pointer entries DMA straight from / to them (no staging).  Same TS -- from the Python
    driver and from the C++ thread-per-block driver."""
    import subprocess, json
    from conftest import host_example
    const, cr, mode_t = g.QAM64, g.C7_8, g.T8k
    c = po.cfg(const, cr, mode_t)
    iq = po.stream_slice(c, 3, 9)
    ref = po.rx(c, iq, want=("ts",))["ts"]
    fg = RxFlowgraph(const, cr, mode_t, len(iq), mode="host", call_symbols=64, register_buffers=True)
    ts = fg.run_threaded(iq)
    assert len(fg.registered) == 11                                   # the source and ten output buffers
    fg.close()
    n = min(len(ts), len(ref))
    assert n > 0.9 * len(ref) and (ts[:n] == ref[:n]).all()
    exe = host_example("rx_blocks_bench")
    fin, fout = tmp_path / "bb.cf32", tmp_path / "out.ts"
    iq.tofile(fin)
    out = subprocess.check_output([exe, "8k", "qam64", "7/8", str(fin), str(fout), "64", "1", "1"], text=True)
    assert json.loads(out.strip().splitlines()[-1])["registered_buffers"] is True
    ts = np.fromfile(fout, np.uint8)
    n = min(len(ts), len(ref))
    assert n > 0.9 * len(ref) and (ts[:n] == ref[:n]).all()


FG_SWEEP = [  # (mode_t, guard, constellation, code rate, driver mode, call_symbols)
    (g.T2k, g.G1_16, g.QPSK, g.C2_3, "device", 1),
    (g.T8k, g.G1_16, g.QAM16, g.C3_4, "host", 4),
    (g.T2k, g.G1_8, g.QAM64, g.C5_6, "device", 33),
    (g.T8k, g.G1_8, g.QPSK, g.C5_6, "device", 4),
    (g.T2k, g.G1_4, g.QAM16, g.C3_4, "host", 33),
    (g.T8k, g.G1_4, g.QAM64, g.C2_3, "device", 1),
]
FG_HIER = [  # (mode_t, guard, constellation, hierarchy, HP rate, LP rate, driver mode, call_symbols)
    (g.T2k, g.G1_16, g.QAM16, g.ALPHA2, g.C1_2, g.C3_4, "device", 4),
    (g.T8k, g.G1_8, g.QAM64, g.ALPHA4, g.C2_3, g.C1_2, "host", 33),
]


@pytest.mark.parametrize("mode_t,guard,const,cr,mode,call_symbols", FG_SWEEP,
                         ids=[f"{'28'[a[0]]}k-g{a[1]}-c{a[2]}-r{a[3]}-{a[4]}-{a[5]}" for a in FG_SWEEP])
def test_block_by_block_every_guard_constellation_rate(po, mode_t, guard, const, cr, mode, call_symbols):
    """the drop-in path at guards 1/16, 1/8, 1/4, QPSK and rates 2/3, 3/4, 5/6 (the blocks get the guard from RxFlowgraph): the oracle's TS from the
    first byte"""
    c = po.cfg(const, cr, mode_t, guard=guard)
    iq = po.stream_slice(c, 3 if mode_t == g.T2k else 2, 9)
    ref = po.rx(c, iq, want=("ts",))["ts"]
    fg = RxFlowgraph(const, cr, mode_t, len(iq), mode=mode, call_symbols=call_symbols, guard=guard)
    ts = fg.run(iq)
    calls = [st.calls for st in fg.stages]
    fg.close()
    assert min(calls) > 0
    n = min(len(ts), len(ref))
    assert n > 0.9 * len(ref) and abs(len(ts) - len(ref)) <= 64 * 1504
    assert (ts[:n] == ref[:n]).all()


@pytest.mark.parametrize("mode_t,guard,const,hier,cr,cr_lp,mode,call_symbols", FG_HIER,
                         ids=[f"{'28'[a[0]]}k-g{a[1]}-c{a[2]}-h{a[3]}-{a[6]}-{a[7]}" for a in FG_HIER])
def test_block_by_block_hierarchical(po, mode_t, guard, const, hier, cr, cr_lp, mode, call_symbols):
    """a hierarchical stream through the drop-in path: no TS comes out (the decoder unpacks d_m bits of every byte of the high-priority stream, as
    gr-dvbt's does: test_gpu_chain.py::test_hierarchical_modes_every_tap), so every stage up to the decoder is held to the oracle over the common
    prefix -- equalised carriers within the contract's tolerance, demap, symbol and bit de-interleaver (output 0) and Viterbi bytes equal"""
    c = po.cfg(const, cr, mode_t, guard=guard, hierarchy=hier)
    pps = po.packets_per_superframe(c)
    iq = po.tx(c, po.make_ts(2 * pps + pps // 2, 14), lead_in=1000, tail=3 * c.N)
    o = po.rx(c, iq, want=("eq", "demap", "symdeint", "bitdeint", "vit"))
    fg = RxFlowgraph(const, cr, mode_t, len(iq), mode=mode, call_symbols=call_symbols, guard=guard, hierarchy=hier, code_rate_lp=cr_lp)
    fg.run(iq)

    def items(k, dtype, width):
        st = fg.stages[k]
        buf = st.out[:st.produced * st.out_item]
        buf = buf.cpu().numpy() if mode == "device" else np.asarray(buf)
        return buf.view(dtype).reshape(-1, width)
    eq = items(2, np.complex64, c.payload)
    taps = {"demap": items(3, np.uint8, c.payload), "symdeint": items(4, np.uint8, c.payload), "bitdeint": items(5, np.uint8, c.payload),
            "vit": items(6, np.uint8, 1).reshape(-1)}
    fg.close()
    ne = min(len(eq), len(o["eq"]))
    assert ne > 0.9 * len(o["eq"]) > 100
    d = eq[:ne] - o["eq"][:ne]
    assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= 1e-3 * 2 * c.norm
    assert taps["bitdeint"].max() == 3                                  # two bits per carrier on the high-priority stream
    for key, a in taps.items():
        b = o[key]
        n = min(len(a), len(b))
        assert n > 0.9 * len(b) > 0, key
        assert (a[:n] == b[:n]).all(), key
