"""What the channel sounder costs (dvbt_sounder_push_device) on the headline workload's symbols: 65 superframes of 8k QAM64 7/8 from the GPU modulator, the
cyclic prefixes dropped and transformed by the FFT block (dvbt_fft_work_device) into fft-shifted rows in device memory, pushed in one call with synthetic
index / offset / cp_start arrays; and, in the same session, what the FFT block takes over the same rows.

  python tools/sounder_bench.py [--out FILE] [--superframes 65] [--iters 20] [--warmup 3] [--what sounder|fft|both]

As one JSON document: the HIP-event time of the push (median, min, max of --iters calls behind --warmup; the handle is reset before each, outside the timed
span), the FFT block's time, their ratio, and the share of the achievable HBM rate at which the rows' bytes (8 N a symbol: the most the sounder reads) pass.
--what sounder or fft runs one of the two and writes no file: the form a counter run (rocprofv3 --pmc ... -- python tools/sounder_bench.py --what sounder)
takes.  Measurement aids live here; bench.py and the package read no environment variable."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s (VERDICT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sounder_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", choices=("sounder", "fft", "both"), default="both")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    if g.device_count() <= 0:
        raise SystemExit("sounder_bench needs a GPU: libdvbt_hip has no CPU fallback")
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    N, cp = c.N, c.cp
    npk = a.superframes * po.packets_per_superframe(c)
    nsym = 272 * a.superframes
    dev = torch.device("cuda:0")
    ts = torch.from_numpy(po.stream_ts(c, 0, a.superframes, 77)).to(dev)
    x = torch.zeros(2 * nsym * (N + cp), dtype=torch.float32, device=dev)
    tx = g.Tx(g.QAM64, g.C7_8, g.T8k, scale=po.tx_scale(c), max_packets=npk)
    nbody = tx.run_device(ts.data_ptr(), npk, x.data_ptr(), nsym * (N + cp))
    torch.cuda.synchronize()
    tx.close()
    assert nbody == nsym * (N + cp)
    items = x.view(nsym, N + cp, 2)[:, cp:, :].contiguous()                     # the cyclic prefixes dropped
    del x
    rows = torch.empty_like(items)
    ints = torch.stack([torch.arange(nsym, dtype=torch.int32) % 68, torch.zeros(nsym, dtype=torch.int32), torch.full((nsym,), 1234, dtype=torch.int32)]).to(dev)
    blk = g.Block("fft", N, 1, 1)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        blk.work_device(nsym, nsym, items.data_ptr(), rows.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes from dvbt_tx_run_device through dvbt_fft_work_device, dvbt_sounder_push_device in one call (Hann)",
           "symbols": int(nsym), "row_bytes": int(8 * N * nsym), "iters": a.iters, "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}
    if a.what in ("sounder", "both"):
        s = g.Sounder(g.T8k, "hann")
        p = [ints[i].data_ptr() for i in range(3)]
        ms = timed(stream, a.iters, a.warmup, s.reset, lambda: s.push_device(rows.data_ptr(), nsym, p[0], p[1], p[2], stream=stream.cuda_stream))
        r = s.read()
        s.close()
        assert (r.symbols_pushed, r.groups_used, r.groups_skipped) == (nsym, nsym // 4, 0)
        med = float(np.median(ms))
        rate = 8.0 * N * nsym / (med * 1e-3)
        out.update({"sounder_median_ms": med, "sounder_min_ms": float(min(ms)), "sounder_max_ms": float(max(ms)), "sounder_us_per_symbol": med * 1e3 / nsym,
                    "gbytes_per_s": rate / 1e9, "fraction_of_hbm_rate": rate / HBM_ACHIEVABLE})
        m0 = int(np.argmax(r.pdp))
        far = np.ones(r.M, bool)
        far[(m0 + np.arange(-4, 5)) % r.M] = False
        out["reading"] = {"paths": r.paths(), "largest_bin_elsewhere_db": float(10 * np.log10(r.pdp[far].max() / r.pdp[m0])), "ripple_db": r.ripple_db(),
                          "groups_used": r.groups_used}
    if a.what in ("fft", "both"):
        ms = timed(stream, a.iters, a.warmup, lambda: None,
                   lambda: blk.work_device(nsym, nsym, items.data_ptr(), rows.data_ptr(), stream=stream.cuda_stream))
        med = float(np.median(ms))
        out.update({"fft_median_ms": med, "fft_min_ms": float(min(ms)), "fft_max_ms": float(max(ms)), "fft_us_per_item": med * 1e3 / nsym})
    blk.close()
    if a.what == "both":
        out["sounder_over_fft"] = out["sounder_median_ms"] / out["fft_median_ms"]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
