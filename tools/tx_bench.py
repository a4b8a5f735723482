"""Throughput of the GPU modulator (dvbt_tx_run_device): 8k QAM64 7/8 GI 1/32, 65 superframes per call (343,980 packets -> 17,680
symbols = 149,360,640 samples), the TS resident in device memory, the baseband written to device memory.  Every call continues the same
stream (the handle carries its state); the packets of each call are the same 65 superframes.  Prints one JSON line: the median time per
call over the timed calls (HIP events), Msamples/s, the multiple of real time (64/7 Msps), and the fraction of the HBM peak that the
compulsory bytes (188 B per packet read + 8 B per sample written) would take at that time; beside it the oracle's single-threaded C
generator (o_tx_generate_from) on the same TS.

    python tools/tx_bench.py [--superframes 65] [--calls 60] [--warmup 5] [--no-oracle]
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
from oracle import pyoracle as po  # noqa: E402

REAL_TIME_MSPS = 64.0 / 7.0
HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec, as bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    if a.calls < 50:
        ap.error("--calls must be >= 50")
    const, cr, mode, guard = g.QAM64, g.C7_8, g.T8k, g.G1_32
    c = po.cfg(const, cr, mode, guard=guard)
    npk = a.superframes * po.packets_per_superframe(c)
    ts = po.stream_ts(c, 0, a.superframes, 1)
    dev = torch.device("cuda:0")
    dts = torch.from_numpy(ts).to(dev)
    tx = g.Tx(const, cr, mode, guard=guard, max_packets=npk)
    nsamp = tx.samples_for(npk)                      # a whole number of superframes: every call gives the same count
    out = torch.empty(2 * nsamp, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    for _ in range(a.warmup):                        # every shape the timed calls use
        assert tx.run_device(dts.data_ptr(), npk, out.data_ptr(), nsamp, stream=s) == nsamp
    stream.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    with torch.cuda.stream(stream):
        for e0, e1 in ev:
            e0.record(stream)
            tx.run_device(dts.data_ptr(), npk, out.data_ptr(), nsamp, stream=s)
            e1.record(stream)
    stream.synchronize()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    med = float(np.median(ms))
    # correctness of the timed path: the first call of a fresh stream against the oracle's generator on the same TS
    tx.reset()
    tx.run_device(dts.data_ptr(), npk, out.data_ptr(), nsamp, stream=s)
    stream.synchronize()
    got = out.cpu().numpy().view(np.complex64)
    res = {"workload": "tx 8k qam64 7/8 gi 1/32", "superframes_per_call": a.superframes, "packets_per_call": int(npk),
           "samples_per_call": int(nsamp), "calls": a.calls, "median_ms_per_call": round(med, 4),
           "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
           "msamples_per_s": round(nsamp / med / 1e3, 1), "x_real_time": round(nsamp / med / 1e3 / REAL_TIME_MSPS, 1),
           "compulsory_bytes": int(npk * 188 + nsamp * 8)}
    res["hbm_fraction"] = round(res["compulsory_bytes"] / (med * 1e-3) / (HBM_PEAK_GBS * 1e9), 3)
    if not a.no_oracle:
        t0 = time.perf_counter()
        ref = po.tx(c, ts, scale=g.TX_SCALE)
        t_or = time.perf_counter() - t0
        res["oracle_s"] = round(t_or, 2)
        res["oracle_msamples_per_s"] = round(len(ref) / t_or / 1e6, 2)
        res["speedup_vs_oracle"] = round(t_or * 1e3 / med, 1)
        res["max_abs_err_rel_peak"] = float(np.abs(got - ref).max() / np.abs(ref).max())
        res["verified"] = bool(len(ref) == nsamp and res["max_abs_err_rel_peak"] <= 1e-5)
    tx.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
