"""What the sample-clock offset block costs (dvbt_clock_run_device) on the headline workload's baseband: 65 superframes of 8k QAM64 7/8 = 149,386,216
samples from the GPU modulator, input and output in device memory, one call = one kernel launch.

  python tools/clock_bench.py [--out FILE] [--superframes 65] [--iters 20] [--warmup 3] [--no-oracle] [--only SETTING]

Three settings: 16, 32 and 64 taps at 10 ppm.  For each, as one JSON document: the HIP-event time of the call (median, min, max of --iters calls behind
--warmup), the rate at the 16 bytes a sample has to move (8 read, 8 written), the fraction of the achievable HBM rate that makes, and beside it the time of
oracle/pyoracle.py::clock_offset (numpy, one host core) with the same taps on 1/64 of the samples on the same machine.
--only runs one setting without the oracle and writes no file: the form a counter run (rocprofv3 --pmc ... -- python tools/clock_bench.py --only taps16)
takes.  Measurement aids live here; bench.py and the package read no environment variable."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s (VERDICT)
BYTES_PER_SAMPLE = 16
PPM = 10.0
SETTINGS = {"taps16": 16, "taps32": 32, "taps64": 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clock_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--only", choices=sorted(SETTINGS), default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    if g.device_count() <= 0:
        raise SystemExit("clock_bench needs a GPU: libdvbt_hip has no CPU fallback")
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    npk = a.superframes * po.packets_per_superframe(c)
    lead = po.STREAM_LEAD_IN
    total = po.stream_len(c, a.superframes)
    dev = torch.device("cuda:0")
    ts = torch.from_numpy(po.stream_ts(c, 0, a.superframes, 77)).to(dev)
    x = torch.zeros(2 * total, dtype=torch.float32, device=dev)
    y = torch.empty(2 * total, dtype=torch.float32, device=dev)
    tx = g.Tx(g.QAM64, g.C7_8, g.T8k, scale=po.tx_scale(c), max_packets=npk)
    nbody = tx.run_device(ts.data_ptr(), npk, x.data_ptr() + 8 * lead, total - lead)
    torch.cuda.synchronize()
    tx.close()
    assert lead + nbody + 3 * c.N == total
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes from dvbt_tx_run_device, dvbt_clock_run_device in one call", "samples": int(total),
           "bytes_per_sample": BYTES_PER_SAMPLE, "iters": a.iters, "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "ppm": PPM,
           "settings": {}}
    n_host = total // 64
    host = x[:2 * n_host].cpu().numpy().view(np.complex64) if not (a.no_oracle or a.only) else None
    stream = torch.cuda.Stream()
    for name in ([a.only] if a.only else list(SETTINGS)):
        taps = SETTINGS[name]
        ck = g.ClockOffset(PPM, taps=taps)
        ms, n_out = [], 0
        with torch.cuda.stream(stream):
            for i in range(a.warmup + a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                n_out = ck.run_device(x.data_ptr(), total, y.data_ptr(), total, stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
        ck.close()
        med = float(np.median(ms))
        rate = BYTES_PER_SAMPLE * n_out / (med * 1e-3)
        r = {"taps": taps, "samples_out": int(n_out), "median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "gbytes_per_s": rate / 1e9,
             "msamples_per_s": n_out / (med * 1e-3) / 1e6, "fraction_of_hbm_rate": rate / HBM_ACHIEVABLE}
        if host is not None:
            t0 = time.perf_counter()
            ref = po.clock_offset(host, PPM, taps=taps)
            dt = time.perf_counter() - t0
            r["oracle_clock_offset"] = {"samples": int(len(ref)), "seconds": dt, "msamples_per_s": len(ref) / dt / 1e6,
                                        "gpu_over_oracle_rate": (n_out / (med * 1e-3)) / (len(ref) / dt)}
        out["settings"][name] = r
    if not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
