"""What the fading block costs (dvbt_fading_run_device) on the headline workload's baseband: 65 superframes of 8k QAM64 7/8 = 149,386,216 samples from the
GPU modulator, input and output in device memory, one call = one kernel launch.

  python tools/fading_bench.py [--out FILE] [--superframes 65] [--iters 20] [--warmup 3] [--only SETTING]

Three settings: one static path; COST 207 TU6 at 100 Hz with 16 sinusoids per path; 24 paths with 32 sinusoids each.  For each, as one JSON document: the
HIP-event time of the call (median, min, max of --iters calls behind --warmup), the rate at the 16 bytes a sample has to move (8 read, 8 written) and the
fraction of the achievable HBM rate that makes.  --only runs one setting and writes no file: the form a counter run (rocprofv3 --pmc ... -- python
tools/fading_bench.py --only tu6) takes.  Measurement aids live here; bench.py and the package read no environment variable."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s (VERDICT)
BYTES_PER_SAMPLE = 16
SAMPLE_RATE = 64e6 / 7


def settings(g):
    tu6, dop = g.tu6_paths(100.0, SAMPLE_RATE)
    many = tuple((37 * i % 4099 if i else 0, 0.0, 0.2) for i in range(24))         # 24 scattered paths, delays spread over half the history
    return {"static": dict(paths=((0, 1.0, 0.0),), doppler=0.0, n_sinusoids=16),
            "tu6": dict(paths=tu6, doppler=dop, n_sinusoids=16),
            "paths24": dict(paths=many, doppler=dop, n_sinusoids=32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fading_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("static", "tu6", "paths24"), default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    if g.device_count() <= 0:
        raise SystemExit("fading_bench needs a GPU: libdvbt_hip has no CPU fallback")
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
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes from dvbt_tx_run_device, dvbt_fading_run_device in one call", "samples": int(total),
           "bytes_per_sample": BYTES_PER_SAMPLE, "iters": a.iters, "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "settings": {}}
    stream = torch.cuda.Stream()
    S = settings(g)
    for name in ([a.only] if a.only else list(S)):
        s = S[name]
        fd = g.Fading(seed=5, **s)
        ms = []
        with torch.cuda.stream(stream):
            for i in range(a.warmup + a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fd.run_device(x.data_ptr(), total, y.data_ptr(), stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
        fd.close()
        med = float(np.median(ms))
        rate = BYTES_PER_SAMPLE * total / (med * 1e-3)
        out["settings"][name] = {"n_paths": len(s["paths"]), "n_sinusoids": s["n_sinusoids"], "doppler_cycles_per_sample": s["doppler"],
                                 "median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "gbytes_per_s": rate / 1e9,
                                 "msamples_per_s": total / (med * 1e-3) / 1e6, "fraction_of_hbm_rate": rate / HBM_ACHIEVABLE}
    if not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
