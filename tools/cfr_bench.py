"""What the crest-factor reduction block costs (dvbt_cfr_run_device) on the headline workload's baseband, and what it buys in front of an amplifier.

  python tools/cfr_bench.py [--out FILE] [--superframes 65] [--iters 10] [--warmup 2] [--only SETTING] [--example-superframes 4] [--ibo 6.0]

1. Time.  65 superframes of 8k QAM64 7/8 from the GPU modulator = 17,680 symbols of 8448 samples, input and output in device memory, one call = one
   launch of one workgroup per symbol.  Settings: `pass` (iterations 0: the copy) and os{1,2,4}_it{1,4} at 7 dB over the mean.  A symbol goes through
   T = 1 + 2 os iterations transforms, all on one LDS image.  In the same run the FFT block (dvbt_fft forward, work_device) transforms the same 17,680
   rows of 8192: its time per row is what one transform costs when its row comes from and goes to HBM.  Per setting: the HIP-event time of the call
   (median, min, max), the time per symbol, and `ratio_to_T_fft_rows` = time per symbol / (T x the FFT block's time per row) -- the expectation is <= 1.
2. Effect.  The INTEGRATION 3l example, 8k QAM64 7/8, --example-superframes long: Tx -> [Cfr 7 dB, 2x, 4 iterations] -> RfFrontend (Rapp p = 2 at --ibo dB
   of input back-off over the mean power in front of the Cfr) -> Spectrum (shoulders, PAPR) and -> Rx -> Constellation (MER), with and without the block.
--only runs one setting and writes no file: the form a counter run takes.  Measurement aids live here; bench.py and the package read no environment
variable."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAPR_DB = 7.0
SETTINGS = {"pass": (1, 0)}
SETTINGS.update({f"os{o}_it{i}": (o, i) for o in (1, 2, 4) for i in (1, 4)})


def timed(torch, stream, iters, warmup, call):
    ms = []
    with torch.cuda.stream(stream):
        for i in range(warmup + iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
    return ms


def example(g, po, torch, nsf, ibo):
    """the INTEGRATION 3l chain with and without the block, at one back-off"""
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    dev = torch.device("cuda:0")
    npk = nsf * po.packets_per_superframe(c)
    lead, total = po.STREAM_LEAD_IN, po.stream_len(c, nsf)
    ts = torch.from_numpy(po.stream_ts(c, 0, nsf, 77)).to(dev)
    x = torch.zeros(2 * total, dtype=torch.float32, device=dev)
    y = torch.zeros(2 * total, dtype=torch.float32, device=dev)
    z = torch.zeros(2 * total, dtype=torch.float32, device=dev)
    tx = g.Tx(g.QAM64, g.C7_8, g.T8k, scale=po.tx_scale(c), max_packets=npk)
    nbody = tx.run_device(ts.data_ptr(), npk, x.data_ptr() + 8 * lead, total - lead)
    torch.cuda.synchronize()
    tx.close()
    meter = g.Channel()
    power = meter.power(x.data_ptr() + 8 * lead, nbody)
    cfr = g.Cfr(g.T8k, g.G1_32, g.Cfr.threshold_for(PAPR_DB, power))
    cfr.run_device(x.data_ptr() + 8 * lead, nbody, y.data_ptr() + 8 * lead)
    reading = cfr.read()
    cfr.close()
    amp = g.RfFrontend(sat_amplitude=g.RfFrontend.saturation(ibo, power), smoothness=2.0)
    half_band = 6817 * (64e6 / 7) / 8192 / 2
    spec = g.Spectrum(2048, 1024, "hann")
    out = {"superframes": nsf, "ibo_db": ibo, "threshold_db": PAPR_DB, "oversampling": 2, "iterations": 4,
           "symbols": reading.symbols, "symbols_clipped": reading.symbols_clipped, "samples_over": reading.samples_over,
           "highest_first_iteration_peak_db": reading.peak_db(power)}
    for name, src in (("without", x), ("with", y)):
        spec.reset()
        spec.push_device(src.data_ptr() + 8 * lead, nbody)
        front = spec.read()
        amp.reset()
        amp.run_device(src.data_ptr(), total, z.data_ptr())
        spec.reset()
        spec.push_device(z.data_ptr() + 8 * lead, nbody)
        behind = spec.read()
        rx = g.Rx(g.QAM64, g.C7_8, g.T8k, max_samples=total, quality=True)
        rep = rx.run_device(z.data_ptr(), total)
        con = g.Constellation.from_rx(rx)
        mer = con.read().mer_db
        con.close(); rx.close()
        out[name] = {"mean_power_over_tx": front.mean_power / power, "papr_db_in_front": front.papr_db(), "papr_1e-3_db_in_front": front.papr_db(1e-3),
                     "papr_1e-4_db_in_front": front.papr_db(1e-4), "shoulder_db_in_front": list(front.shoulder_db(half_band)),
                     "papr_db_behind_amplifier": behind.papr_db(), "shoulder_db_behind_amplifier": list(behind.shoulder_db(half_band)),
                     "mer_db_behind_amplifier": float(mer), "rs_fail_words": int(rep.rs_fail_words), "rs_corrected_symbols": int(rep.rs_corrected_symbols)}
    amp.close(); spec.close(); meter.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfr_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=sorted(SETTINGS), default=None)
    ap.add_argument("--example-superframes", type=int, default=4)
    ap.add_argument("--ibo", type=float, default=6.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    if g.device_count() <= 0:
        raise SystemExit("cfr_bench needs a GPU: libdvbt_hip has no CPU fallback")
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    N, S = c.N, c.N + c.cp
    npk = a.superframes * po.packets_per_superframe(c)
    nsym = a.superframes * 4 * 68
    dev = torch.device("cuda:0")
    ts = torch.from_numpy(po.stream_ts(c, 0, a.superframes, 77)).to(dev)
    x = torch.zeros(2 * nsym * S, dtype=torch.float32, device=dev)
    y = torch.empty(2 * nsym * S, dtype=torch.float32, device=dev)
    tx = g.Tx(g.QAM64, g.C7_8, g.T8k, scale=po.tx_scale(c), max_packets=npk)
    nbody = tx.run_device(ts.data_ptr(), npk, x.data_ptr(), nsym * S)
    torch.cuda.synchronize()
    tx.close()
    assert nbody == nsym * S
    meter = g.Channel()
    power = meter.power(x.data_ptr(), nbody)
    meter.close()
    A = g.Cfr.threshold_for(PAPR_DB, power)
    stream = torch.cuda.Stream()
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes from dvbt_tx_run_device, dvbt_cfr_run_device in one call", "symbols": nsym,
           "samples": int(nbody), "threshold_db": PAPR_DB, "iters": a.iters, "warmup": a.warmup, "ref_power": power, "settings": {}}
    # the FFT block on as many rows (the first nsym N samples of the same buffer: its time does not depend on the data)
    fft = g.Block("fft", N, 1, 1)
    ms = timed(torch, stream, a.iters, a.warmup, lambda: fft.work_device(nsym, nsym, x.data_ptr(), y.data_ptr(), stream=stream.cuda_stream))
    fft.close()
    fft_row_us = float(np.median(ms)) * 1e3 / nsym
    out["fft_block"] = {"rows": nsym, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "us_per_row": fft_row_us}
    for name in ([a.only] if a.only else list(SETTINGS)):
        os_, it = SETTINGS[name]
        f = g.Cfr(g.T8k, g.G1_32, A, it, os_)
        ms = timed(torch, stream, a.iters, a.warmup, lambda: f.run_device(x.data_ptr(), nbody, y.data_ptr(), stream=stream.cuda_stream))
        r = f.read()
        f.close()
        calls = a.iters + a.warmup
        assert r.symbols == calls * nsym and r.symbols_nonfinite == 0
        med = float(np.median(ms))
        T = 1 + 2 * os_ * it if it else 0
        row = {"oversampling": os_, "iterations": it, "transforms_per_symbol": T, "median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)),
               "us_per_symbol": med * 1e3 / nsym, "msamples_per_s": nbody / (med * 1e-3) / 1e6, "symbols_clipped_per_call": r.symbols_clipped // calls,
               "samples_over_per_call": r.samples_over // calls}
        if T:
            row["us_per_transform"] = med * 1e3 / nsym / T
            row["ratio_to_T_fft_rows"] = med * 1e3 / nsym / (T * fft_row_us)
        out["settings"][name] = row
    del x, y
    if not a.only:
        out["example"] = example(g, po, torch, a.example_superframes, a.ibo)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
