"""What the signal scanner costs (dvbt_scan_push_device) on the headline workload's baseband: 65 superframes of 8k QAM64 7/8 from the GPU modulator, in
device memory, pushed in one call -- the whole stream, and its first 1,048,576 samples (a realistic scan); and, in the same session, what a pass that reads
and writes the same buffer takes (dvbt_rf_run_device with every stage off) and what dvbt_spectrum_push_device takes at N = 8192, hop N.

  python tools/scan_bench.py [--out FILE] [--superframes 65] [--iters 20] [--warmup 3] [--only whole|head]

As one JSON document: the HIP-event time of each (median, min, max of --iters calls behind --warmup; the handles are reset before each, outside the timed
span), the two ratios, and the rate at the 8 bytes a sample occupies -- the scanner reads every sample at 16 places (a and b of eight hypotheses) plus once to
count the non-finite ones, so that rate is not a share of the HBM rate unless the other reads come from the caches.  --only runs the scanner alone on one
length and writes no file: the form a counter run takes.
Measurement aids live here; bench.py and the package read no environment variable."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s (VERDICT)
HEAD = 1 << 20


def timed(stream, iters, warmup, before, call):
    import torch
    ms = []
    with torch.cuda.stream(stream):
        for i in range(warmup + iters):
            before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms, samples, bytes_per_sample):
    import numpy as np
    med = float(np.median(ms))
    return {"samples": int(samples), "median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "msamples_per_s": samples / (med * 1e-3) / 1e6,
            "gbytes_per_s": bytes_per_sample * samples / (med * 1e-3) / 1e9, "bytes_per_sample_counted": bytes_per_sample,
            "fraction_of_hbm_rate": bytes_per_sample * samples / (med * 1e-3) / HBM_ACHIEVABLE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("whole", "head"), default=None)
    a = ap.parse_args()
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    if g.device_count() <= 0:
        raise SystemExit("scan_bench needs a GPU: libdvbt_hip has no CPU fallback")
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    npk = a.superframes * po.packets_per_superframe(c)
    lead = po.STREAM_LEAD_IN
    total = po.stream_len(c, a.superframes)
    dev = torch.device("cuda:0")
    ts = torch.from_numpy(po.stream_ts(c, 0, a.superframes, 77)).to(dev)
    x = torch.zeros(2 * total, dtype=torch.float32, device=dev)
    tx = g.Tx(g.QAM64, g.C7_8, g.T8k, scale=po.tx_scale(c), max_packets=npk)
    nbody = tx.run_device(ts.data_ptr(), npk, x.data_ptr() + 8 * lead, total - lead)
    torch.cuda.synchronize()
    tx.close()
    assert lead + nbody + 3 * c.N == total
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes from dvbt_tx_run_device, dvbt_scan_push_device in one call", "iters": a.iters,
           "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}
    stream = torch.cuda.Stream()
    sc = g.Scanner()
    for name, n in (("whole", total), ("head", min(HEAD, total))):
        if a.only and a.only != name:
            continue
        ms = timed(stream, a.iters, a.warmup, sc.reset, lambda: sc.push_device(x.data_ptr(), n, stream=stream.cuda_stream))
        r = sc.read()
        assert r.samples_pushed == n and r.detected and (r.mode, r.guard) == (g.T8k, g.G1_32), r
        out["scan_" + name] = stats(ms, n, 8.0)
        out["scan_" + name]["reading"] = {"rho": r.rho, "symbol_start": r.symbol_start[4], "cfo": r.cfo[4], "symbols": r.symbols}
    sc.close()
    if not a.only:
        y = torch.empty_like(x)
        rf = g.RfFrontend()                                                # every stage off: the pass reads and writes the buffer
        ms = timed(stream, a.iters, a.warmup, lambda: None, lambda: rf.run_device(x.data_ptr(), total, y.data_ptr(), stream=stream.cuda_stream))
        rf.close()
        del y
        out["rf_all_off"] = stats(ms, total, 16.0)
        sp = g.Spectrum(8192, 8192, "hann")
        ms = timed(stream, a.iters, a.warmup, sp.reset, lambda: sp.push_device(x.data_ptr(), total, stream=stream.cuda_stream))
        sp.close()
        out["spectrum_8k_full"] = stats(ms, total, 8.0)
        out["scan_over_rf_all_off"] = out["scan_whole"]["median_ms"] / out["rf_all_off"]["median_ms"]
        out["scan_over_spectrum_8k_full"] = out["scan_whole"]["median_ms"] / out["spectrum_8k_full"]["median_ms"]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
