"""What the tuner block costs (dvbt_tuner_run_device) for the headline workload's baseband at its OUTPUT: 65 superframes of 8k QAM64 7/8 = 149,386,216
complex64 samples out, raw input and output in device memory, one call = one kernel launch.

  python tools/tuner_bench.py [--out FILE] [--superframes 65] [--iters 20] [--warmup 3] [--only CASE]

Cases: cs16, cs8 and cf32 at 32/35 (a 10 Msps capture) with the designed taps; cs16_shift (the same with the mixer on); cs16_16_35 (a 20 Msps capture);
cf32_rs_taps (CF32 at 64/70 with the taps and scale of the pinned resampler block) and, as the yardstick from before the tuner, resampler: the pinned
block's dvbt_resampler_work_device on the same CF32 input.  The input is seeded noise made on the device (the kernel's time does not depend on the values:
no branch and no denormal is reached through them).  The cases are timed in turn inside one loop, so that whatever else the machine does falls on all
of them alike.  For each, as one JSON document: the HIP-event time of the call (median, min, max of --iters calls behind --warmup), the bytes a call has
to move (raw bytes x M / L + 8 per output), the rate and the fraction of the achievable HBM rate that makes; then the two ratios the block is held to
(cf32_rs_taps over resampler, cs16 over cf32) beside the spread of each side's own repeats.
--only runs one case and writes no file: the form a counter run (rocprofv3 --pmc ... -- python tools/tuner_bench.py --only cs16) takes.  Measurement aids
live here; bench.py and the package read no environment variable."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s (VERDICT)
RS_SCALE = 0.00055242272      # multiply_const behind the resampler in the reference's receive flowgraph
SHIFT = -0.025                # a channel 250 kHz above the centre of a 10 Msps capture
CASES = ("cs16", "cs8", "cf32", "cs16_shift", "cs16_16_35", "cf32_rs_taps", "resampler")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuner_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=CASES, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    if g.device_count() <= 0:
        raise SystemExit("tuner_bench needs a GPU: libdvbt_hip has no CPU fallback")
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    n_out = po.stream_len(c, a.superframes)
    dev = torch.device("cuda:0")
    names = [a.only] if a.only else list(CASES)

    def inputs_for(L, M):
        return -(-n_out * M // L)                 # the fewest inputs that complete n_out outputs ... or one more: the call's count is read back

    n10, n20 = inputs_for(32, 35), inputs_for(16, 35)
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    bufs = {}
    if any(n in names for n in ("cf32", "cf32_rs_taps", "resampler")):
        bufs["cf32"] = torch.randn(2 * n10, dtype=torch.float32, device=dev, generator=gen)
    if any(n.startswith("cs16") for n in names):
        bufs["cs16"] = torch.randint(-32768, 32768, (2 * max(n10, n20 if "cs16_16_35" in names else 0),), dtype=torch.int16, device=dev, generator=gen)
    if "cs8" in names:
        bufs["cs8"] = torch.randint(-128, 128, (2 * n10,), dtype=torch.int8, device=dev, generator=gen)
    y = torch.empty(2 * (n_out + 64), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()

    rs = g.Block("resampler", 64, 70, RS_SCALE)
    fn = rs.L.dvbt_resampler_get_taps
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    rs_taps = np.zeros(fn(rs.h, None, 0, None, None), np.float32)
    fn(rs.h, rs_taps.ctypes.data_as(C.c_void_p), len(rs_taps), None, None)

    def tuner_case(fmt, L, M, src, n_in, **kw):
        t = g.Tuner(fmt, L, M, **kw)

        def call():
            return t.run_device(bufs[src].data_ptr(), n_in, y.data_ptr(), n_out + 64, stream=stream.cuda_stream)
        return dict(call=call, close=t.close, raw_bytes=g.IQ_BYTES[fmt], L=t.desc.interpolation, M=t.desc.decimation, n_in=n_in, nt=t.desc.nt, ntaps=t.desc.ntaps)

    def resampler_case():
        def call():
            return rs.work_device(n_out, n10, bufs["cf32"].data_ptr(), y.data_ptr(), stream=stream.cuda_stream)[0]
        return dict(call=call, close=lambda: None, raw_bytes=8, L=32, M=35, n_in=n10, nt=-(-len(rs_taps) // 32), ntaps=len(rs_taps))

    make = {
        "cs16": lambda: tuner_case(g.IQ_CS16, 32, 35, "cs16", n10),
        "cs8": lambda: tuner_case(g.IQ_CS8, 32, 35, "cs8", n10),
        "cf32": lambda: tuner_case(g.IQ_CF32, 32, 35, "cf32", n10),
        "cs16_shift": lambda: tuner_case(g.IQ_CS16, 32, 35, "cs16", n10, shift=SHIFT),
        "cs16_16_35": lambda: tuner_case(g.IQ_CS16, 16, 35, "cs16", n20),
        "cf32_rs_taps": lambda: tuner_case(g.IQ_CF32, 64, 70, "cf32", n10, taps=rs_taps, scale=RS_SCALE),
        "resampler": resampler_case,
    }
    cases = {n: make[n]() for n in names}
    ms = {n: [] for n in names}
    counts = {}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for i in range(a.warmup + a.iters):
            for n in names:                       # in turn: the cases share whatever else the machine is doing
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                counts[n] = cases[n]["call"]()
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    ms[n].append(e0.elapsed_time(e1))
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes at the output, dvbt_tuner_run_device in one call on seeded noise", "samples_out": int(n_out),
           "iters": a.iters, "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "shift": SHIFT, "cases": {}}
    for n in names:
        k = cases[n]
        k["close"]()
        med, produced = float(np.median(ms[n])), int(counts[n])
        per_out = k["raw_bytes"] * k["M"] / k["L"] + 8
        rate = per_out * produced / (med * 1e-3)
        out["cases"][n] = {"ratio": f"{k['L']}/{k['M']}", "raw_bytes_per_sample": k["raw_bytes"], "ntaps": k["ntaps"], "taps_per_branch": k["nt"],
                           "samples_in": int(k["n_in"]), "samples_out": produced, "median_ms": med, "min_ms": float(min(ms[n])), "max_ms": float(max(ms[n])),
                           "spread": (max(ms[n]) - min(ms[n])) / med, "bytes_per_output": per_out, "gbytes_per_s": rate / 1e9,
                           "msamples_out_per_s": produced / (med * 1e-3) / 1e6, "fraction_of_hbm_rate": rate / HBM_ACHIEVABLE}
    rs.close()

    def ratio(x, over):
        if x in out["cases"] and over in out["cases"]:
            r = out["cases"][x]["median_ms"] / out["cases"][over]["median_ms"]
            s = max(out["cases"][x]["spread"], out["cases"][over]["spread"])
            return {"time_ratio": r, "largest_spread_of_either": s, "no_slower_beyond_the_spread": bool(r <= 1.0 + s)}
        return None
    out["expectations"] = {"cf32_rs_taps_over_resampler": ratio("cf32_rs_taps", "resampler"), "cs16_over_cf32": ratio("cs16", "cf32")}
    if not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
