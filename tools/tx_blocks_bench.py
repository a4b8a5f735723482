"""The transmit blocks one at a time (dvbt_<blk>_work_device) at the item sizes of apps/dvbt_tx_demo_8k_QAM64_rate78.grc, over the workload of
tools/tx_bench.py: 8k QAM64 7/8 GI 1/32, 65 superframes (343,980 packets -> 17,680 symbols).  Every block gets the whole workload in one call
(symbol_inner_interleaver, which takes at most 4096 items per call, in five), on device buffers filled by the block in front of it; the time is
the median over --reps repetitions (HIP events), and beside it the compulsory bytes (input read + output written once) at the HBM peak.  Then the
whole TxFlowgraph in device mode (calls of --call-items output multiples, the cyclic prefix and the scale in torch) against dvbt_tx_run_device
on the same TS.  Prints one JSON object.

    python tools/tx_blocks_bench.py [--superframes 65] [--reps 10] [--call-items 512]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gr_dvbt_amd as g  # noqa: E402
from gr_dvbt_amd.flowgraph import TxFlowgraph  # noqa: E402

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec, as bench.py and tools/tx_bench.py


def _ms(fn, reps, stream):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--call-items", type=int, default=512)
    a = ap.parse_args()
    const, cr, mode, guard = g.QAM64, g.C7_8, g.T8k, g.G1_32
    d = g.get_dims(const, cr, mode, guard)
    N, P, ib = d.fft_length, d.payload_length, d.info_bits_per_symbol
    nsym = a.superframes * 272
    npk = nsym * ib // 1632
    nb = 4
    items = npk // (8 * nb)                      # energy_dispersal / reed_solomon_enc / convolutional_interleaver items (6016, 6528 B)
    rng = np.random.default_rng(1)
    ts = rng.integers(0, 256, (npk, 188), dtype=np.uint8)
    ts[:, 0] = 0x47
    ts = ts.reshape(-1)
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    dev = lambda nbytes: torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
    d_ts = torch.from_numpy(ts).cuda()
    coded = items * 1632 * nb
    nsym_c = coded * 8 * d.cr_n // (d.cr_k * d.m) // P // 4 * 4
    bufs = {"ed": dev(items * 1504 * nb), "rs": dev(items * 1632 * nb), "ci": dev(coded), "ic": dev(nsym_c * P), "bi": dev(nsym_c * P),
            "si": dev(nsym_c * P), "map": dev(nsym_c * P * 8), "ref": dev(nsym_c * N * 8), "fft": dev(nsym_c * N * 8)}
    torch.cuda.synchronize()
    B = g.Block
    # (name, block, nout, nin, input, output, compulsory bytes)
    plan = [
        ("energy_dispersal", B("energy_dispersal", nb), items, len(ts), d_ts, bufs["ed"], 2 * items * 1504 * nb),
        ("reed_solomon_enc", B("reed_solomon_enc", 2, 8, 0x11d, 255, 239, 8, 51, 8 * nb), items, items, bufs["ed"], bufs["rs"], items * (1504 + 1632) * nb),
        ("convolutional_interleaver", B("convolutional_interleaver", 136 * nb, 12, 17), coded, items, bufs["rs"], bufs["ci"], 2 * coded),
        ("inner_coder", B("inner_coder", 1, P, const, g.NH, cr), nsym_c, coded, bufs["ci"], bufs["ic"], coded + nsym_c * P),
        ("bit_inner_interleaver", B("bit_inner_interleaver", P, const, g.NH, mode), nsym_c, nsym_c, bufs["ic"], bufs["bi"], 2 * nsym_c * P),
        ("symbol_inner_interleaver", B("symbol_inner_interleaver", P, mode, 1), nsym_c, nsym_c, bufs["bi"], bufs["si"], 2 * nsym_c * P),
        ("map", B("map", P, const, g.NH, mode, 1.0), nsym_c, nsym_c, bufs["si"], bufs["map"], nsym_c * P * 9),
        ("reference_signals", B("reference_signals", 8, P, N, const, g.NH, cr, cr, guard, mode, 0, 0), nsym_c, nsym_c, bufs["map"], bufs["ref"],
         nsym_c * (P + N) * 8),
        ("fft", B("fft", N, 0, 1), nsym_c, nsym_c, bufs["ref"], bufs["fft"], 2 * nsym_c * N * 8),
    ]
    in_item = {"symbol_inner_interleaver": P}
    out = {"workload": "tx blocks 8k qam64 7/8 gi 1/32", "superframes": a.superframes, "packets": npk, "symbols": nsym_c, "reps": a.reps, "blocks": []}
    total = 0.0
    for name, blk, nout, nin, src, dst, cbytes in plan:
        def call(blk=blk, nout=nout, nin=nin, src=src, dst=dst, name=name):
            if name == "symbol_inner_interleaver":                    # at most 4096 items per call
                for o in range(0, nout, 4096):
                    n = min(4096, nout - o)
                    blk.work_device(n, n, src.data_ptr() + o * in_item[name], dst.data_ptr() + o * P, (), sp)
            else:
                r, cons, _ = blk.work_device(nout, nin, src.data_ptr(), dst.data_ptr(), (), sp)
                assert r > 0, name
        call()                                                        # warm-up
        st.synchronize()
        ms = _ms(call, a.reps, st)
        total += ms
        floor = cbytes / (HBM_PEAK_GBS * 1e9) * 1e3
        out["blocks"].append({"block": name, "ms": round(ms, 4), "compulsory_bytes": int(cbytes), "ms_at_hbm_peak": round(floor, 4),
                              "x_hbm_floor": round(ms / floor, 2)})
        blk.close()
    out["sum_of_blocks_ms"] = round(total, 3)

    # the whole flowgraph (device mode) against the fused modulator on the same TS
    def fg_run():
        fg = TxFlowgraph(const, cr, mode, guard=guard, mode="device", call_items=a.call_items)
        fg.stream = st
        bb, _ = fg.run(ts, to_host=False)
        st.synchronize()
        fg.close()
        return bb
    fg_run()
    t = []
    for _ in range(max(3, a.reps // 3)):
        t0 = time.perf_counter()
        bb = fg_run()
        t.append((time.perf_counter() - t0) * 1e3)
    out["flowgraph_device_ms"] = round(float(np.median(t)), 3)
    out["flowgraph_call_items"] = a.call_items
    tx = g.Tx(const, cr, mode, guard=guard, max_packets=npk)
    cap = tx.samples_for(npk)
    iq = torch.empty(cap * 8 + 64, dtype=torch.uint8, device="cuda")

    def fused():
        tx.reset()
        tx.run_device(d_ts.data_ptr(), npk, iq.data_ptr(), cap, sp)
    fused()
    st.synchronize()
    out["fused_ms"] = round(_ms(fused, a.reps, st), 4)
    n = bb.numel()
    ref = iq[:cap * 8].view(torch.complex64)[:n]
    out["flowgraph_samples"] = int(n)
    out["flowgraph_max_err_rel_peak"] = float(((bb - ref).abs().max() / ref.abs().max()).item())
    out["chain_blocks_over_fused"] = round(total / out["fused_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
