"""What the constellation analyser costs (dvbt_constellation_push_device) on the headline workload's equalised cells: 17,680 rows of 6048 cells -- 65 superframes
of 8k QAM64 7/8 -- in device memory, pushed in one call; and, in the same session, what dvbt_rf_run_device with every stage off takes over the same number of
complex64 (a pass that reads and writes the buffer, 16 bytes a sample).

  python tools/constellation_bench.py [--out FILE] [--superframes 65] [--iters 20] [--warmup 3] [--what clean|noisy|uniform|rf|all]

Three inputs, because they stress different things: `clean` cells on the 64 points themselves (every cell of a wavefront meets the others on 64 counters),
`noisy` the same cells with Gaussian error at 20 dB, `uniform` cells spread evenly over the density's span (the most bins touched, the most counters to
flush).  As one JSON document: per input the HIP-event time of the push (median, min, max of --iters calls behind --warmup; the handle is reset before each,
outside the timed span), the time per cell and the share of the achievable HBM rate at 8 bytes a cell; the RF pass's time; the ratios.  --what with one name
runs that alone and writes no file: the form a counter run (rocprofv3 --pmc ... -- python tools/constellation_bench.py --what clean) takes.  Measurement
aids live here; bench.py and the package read no environment variable."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s (VERDICT)
INPUTS = ("clean", "noisy", "uniform")


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


def make_cells(torch, kind, nrows, P, dev):
    """[nrows][P][2] float32 on the device"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    d = float(1.0 / 42.0 ** 0.5)
    if kind == "uniform":
        return ((torch.rand((nrows, P, 2), generator=gen, device=dev) * 2.0 - 1.0) * (8.0 * d)).contiguous()
    x = (torch.randint(0, 8, (nrows, P, 2), generator=gen, device=dev).to(torch.float32) * 2.0 - 7.0) * d
    if kind == "noisy":
        x += torch.randn((nrows, P, 2), generator=gen, device=dev) * (0.5 * 10.0 ** -2.0) ** 0.5
    return x.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constellation_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", choices=INPUTS + ("rf", "all"), default="all")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    if g.device_count() <= 0:
        raise SystemExit("constellation_bench needs a GPU: libdvbt_hip has no CPU fallback")
    P, nrows = 6048, 272 * a.superframes
    cells = nrows * P
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    out = {"workload": f"{nrows} rows of {P} cells (8k QAM64 7/8, {a.superframes} superframes), dvbt_constellation_push_device in one call",
           "rows": nrows, "cells": cells, "cell_bytes": 8 * cells, "iters": a.iters, "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}
    for kind in INPUTS:
        if a.what not in (kind, "all"):
            continue
        x = make_cells(torch, kind, nrows, P, dev)
        torch.cuda.synchronize()
        c = g.Constellation(g.QAM64, g.NH, row_length=P)
        ms = timed(stream, a.iters, a.warmup, c.reset, lambda: c.push_device(x.data_ptr(), nrows, stream=stream.cuda_stream))
        r = c.read()
        c.close()
        assert (r.rows_pushed, r.cells, r.nonfinite) == (nrows, cells, 0) and int(r.hist.sum()) == cells
        med = float(np.median(ms))
        rate = 8.0 * cells / (med * 1e-3)
        out[kind] = {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "ns_per_cell": med * 1e6 / cells, "gbytes_per_s": rate / 1e9,
                     "fraction_of_hbm_rate": rate / HBM_ACHIEVABLE, "bins_touched": int((r.hist > 0).sum()), "mer_db": r.mer_db if np.isfinite(r.mer_db) else None, "clipped": r.clipped}
        del x
    if a.what in ("rf", "all"):
        x = make_cells(torch, "noisy", nrows, P, dev)
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        rf = g.RfFrontend()                                                # every stage off: the pass reads and writes the buffer
        ms = timed(stream, a.iters, a.warmup, lambda: None, lambda: rf.run_device(x.data_ptr(), cells, y.data_ptr(), stream=stream.cuda_stream))
        rf.close()
        med = float(np.median(ms))
        out["rf_all_off"] = {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "fraction_of_hbm_rate": 16.0 * cells / (med * 1e-3) / HBM_ACHIEVABLE}
    if a.what == "all":
        for kind in INPUTS:
            out[kind]["over_rf_all_off"] = out[kind]["median_ms"] / out["rf_all_off"]["median_ms"]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
