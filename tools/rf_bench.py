"""What the RF front-end block costs (dvbt_rf_run_device) on the headline workload's baseband: 65 superframes of 8k QAM64 7/8 = 149,386,216 samples from the
GPU modulator, input and output in device memory, one call = one kernel launch.

  python tools/rf_bench.py [--out FILE] [--superframes 65] [--iters 20] [--warmup 3] [--only SETTING]

Five settings: `off` (every stage off: the streaming pass); `iqdc` (IQ imbalance 0.5 dB / 3 degrees and a DC offset); `pa` (the amplifier at 6 dB input
back-off, p = 2); `pn16` (16 tones of phase noise); `all32` (the amplifier, 32 tones, IQ imbalance and DC).  For each, as one JSON document: the HIP-event
time of the call (median, min, max of --iters calls behind --warmup), the rate at the 16 bytes a sample has to move (8 read, 8 written) and the fraction
of the achievable HBM rate that makes.  --only runs one setting and writes no file: the form a counter run (rocprofv3 --pmc ... -- python
tools/rf_bench.py --only all32) takes.  Measurement aids live here; bench.py and the package read no environment variable."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s (VERDICT)
BYTES_PER_SAMPLE = 16
SAMPLE_RATE = 64e6 / 7
MASK = ((100.0, -60.0), (1e3, -70.0), (1e4, -80.0), (1e5, -100.0), (1e6, -120.0))
NAMES = ("off", "iqdc", "pa", "pn16", "all32")


def settings(g, ref_power):
    mu, nu = g.RfFrontend.iq_imbalance(0.5, 3.0)
    dc = 0.05 * ref_power ** 0.5
    A = g.RfFrontend.saturation(6.0, ref_power)
    return {"off": dict(),
            "iqdc": dict(mu=mu, nu=nu, dc=dc),
            "pa": dict(sat_amplitude=A, smoothness=2.0),
            "pn16": dict(tones=g.phase_noise_tones(MASK, 16, 5, SAMPLE_RATE)),
            "all32": dict(sat_amplitude=A, smoothness=2.0, tones=g.phase_noise_tones(MASK, 32, 5, SAMPLE_RATE), mu=mu, nu=nu, dc=dc)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rf_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=NAMES, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    if g.device_count() <= 0:
        raise SystemExit("rf_bench needs a GPU: libdvbt_hip has no CPU fallback")
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
    meter = g.Channel()
    ref_power = meter.power(x.data_ptr() + 8 * lead, nbody)
    meter.close()
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes from dvbt_tx_run_device, dvbt_rf_run_device in one call", "samples": int(total),
           "bytes_per_sample": BYTES_PER_SAMPLE, "iters": a.iters, "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "ref_power": ref_power, "settings": {}}
    stream = torch.cuda.Stream()
    S = settings(g, ref_power)
    for name in ([a.only] if a.only else list(NAMES)):
        s = S[name]
        fe = g.RfFrontend(**s)
        ms = []
        with torch.cuda.stream(stream):
            for i in range(a.warmup + a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fe.run_device(x.data_ptr(), total, y.data_ptr(), stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
        fe.close()
        med = float(np.median(ms))
        rate = BYTES_PER_SAMPLE * total / (med * 1e-3)
        out["settings"][name] = {"amplifier": bool(s.get("sat_amplitude")), "n_tones": len(s["tones"][0]) if "tones" in s else 0, "iq_dc": "mu" in s,
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
