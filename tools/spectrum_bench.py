"""What the spectrum analyser costs (dvbt_spectrum_push_device) on the headline workload's baseband: 65 superframes of 8k QAM64 7/8 from the GPU modulator,
in device memory, one call; and, in the same session, what the FFT block (dvbt_fft_work_device, fft_items_kernel) takes for as many items of the same size.

  python tools/spectrum_bench.py [--out FILE] [--superframes 65] [--iters 20] [--warmup 3] [--only SETTING [--what spectrum|fft]]

Three settings, all Hann: `8k_half` (N = 8192, hop N/2), `8k_full` (N = 8192, hop N), `2k_full` (N = 2048, hop N).  For each, as one JSON document: the
HIP-event time of the push (median, min, max of --iters calls behind --warmup; the handle is reset before each, outside the timed span), the time per
segment, the FFT block's time per item, their ratio, and the share of the achievable HBM rate at the 8 bytes x N / hop that a sample is read.  --only runs
one setting and writes no file: the form a counter run (rocprofv3 --pmc ... -- python tools/spectrum_bench.py --only 8k_half --what spectrum) takes.
A workgroup sums 32 segments, and two workgroups fit a CU, so the device works through the stream's groups in rounds of 2 x CUs; the 65 superframes are
only 1.1 to 4.5 rounds, and the last, partly empty one counts.  `whole_rounds` is the same measurement on the stream's head cut to whole rounds: the
cost per segment that a long stream sees.
Measurement aids live here; bench.py and the package read no environment variable."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s (VERDICT)
SETTINGS = {"8k_half": (8192, 4096), "8k_full": (8192, 8192), "2k_full": (2048, 2048)}


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


def measure(g, x, total, N, hop, segs, what, stream, iters, warmup):
    """the push of `total` samples (segs segments) and the FFT block over segs items, as a dict of times"""
    import numpy as np
    import torch
    row = {"segments": int(segs)}
    if what in ("spectrum", "both"):
        sp = g.Spectrum(N, hop, "hann")
        ms = timed(stream, iters, warmup, sp.reset, lambda: sp.push_device(x.data_ptr(), total, stream=stream.cuda_stream))
        r = sp.read()
        sp.close()
        assert r.segments == segs
        med = float(np.median(ms))
        rate = 8.0 * total * N / hop / (med * 1e-3)
        row.update({"spectrum_median_ms": med, "spectrum_min_ms": float(min(ms)), "spectrum_max_ms": float(max(ms)), "spectrum_us_per_segment": med * 1e3 / segs,
                    "gbytes_per_s": rate / 1e9, "msamples_per_s": total / (med * 1e-3) / 1e6, "fraction_of_hbm_rate": rate / HBM_ACHIEVABLE})
        row["reading"] = {"mean_power": r.mean_power, "papr_db": float(r.papr_db()), "papr_db_at_1e-4": r.papr_db(1e-4), "occupied_bandwidth_99_hz": r.occupied_bandwidth(0.99)}
    if what in ("fft", "both"):
        # as many items as the analyser has segments: the stream twice over where the segments overlap
        reps = -(-segs * N // (x.numel() // 2))
        fin = x.repeat(reps)[:2 * segs * N].contiguous() if reps > 1 else x
        fout = torch.empty(2 * segs * N, dtype=torch.float32, device=x.device)
        blk = g.Block("fft", N, 1, 1)
        torch.cuda.synchronize()
        ms = timed(stream, iters, warmup, lambda: None, lambda: blk.work_device(int(segs), int(segs), fin.data_ptr(), fout.data_ptr(), stream=stream.cuda_stream))
        blk.close()
        del fin, fout
        med = float(np.median(ms))
        row.update({"fft_median_ms": med, "fft_min_ms": float(min(ms)), "fft_max_ms": float(max(ms)), "fft_us_per_item": med * 1e3 / segs})
    if what == "both":
        row["spectrum_over_fft_per_segment"] = row["spectrum_us_per_segment"] / row["fft_us_per_item"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=sorted(SETTINGS), default=None)
    ap.add_argument("--what", choices=("spectrum", "fft", "both"), default="both")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    if g.device_count() <= 0:
        raise SystemExit("spectrum_bench needs a GPU: libdvbt_hip has no CPU fallback")
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
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes from dvbt_tx_run_device, dvbt_spectrum_push_device in one call (Hann)", "samples": int(total),
           "iters": a.iters, "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "settings": {}}
    stream = torch.cuda.Stream()
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count      # two workgroups of 512 threads per CU (registers; LDS at N = 8192)
    for name in ([a.only] if a.only else list(SETTINGS)):
        N, hop = SETTINGS[name]
        segs = (total - N) // hop + 1
        groups = -(-segs // 32)
        row = {"fft_size": N, "hop": hop, "groups_of_32_segments": int(groups), "workgroup_slots": int(slots), "rounds": groups / slots}
        row.update(measure(g, x, total, N, hop, segs, a.what, stream, a.iters, a.warmup))
        whole = groups // slots * slots                                        # the head of the stream that fills whole rounds
        if whole:
            row["whole_rounds"] = measure(g, x, N + (32 * whole - 1) * hop, N, hop, 32 * whole, a.what, stream, a.iters, a.warmup)
            row["whole_rounds"].pop("reading", None)
        out["settings"][name] = row
    if not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
