"""What the blind signal-quality measurement costs (dvbt_rx_quality) on the headline workload: 8k / QAM64 / 7/8, 65 superframes, one handle.

  python tools/quality_bench.py [--parent-lib PATH] [--out FILE] [--superframes 65] [--iters 20] [--warmup 3]

Records, as one JSON document:
  * the HIP-event time of each of the four kernels (median of --iters launches behind --warmup, dvbt_debug_quality_time), the bytes each reads and
    the fraction of the achievable HBM rate that makes;
  * the host time of the whole dvbt_rx_quality call (launches, synchronisation, read-back);
  * the segment's decode time (dvbt_rx_enable_timing, stage "total") with dvbt_rx_enable_quality off and on -- the price of the symbol kernel's
    instantiation that writes the equalised carriers;
  * with --parent-lib (a build of the commit before the feature, same C ABI): the decode time of the same segment through THAT library, and the ratio
    of the quality call to it.  Every library is measured in a process of its own.
Measurement aids live here; bench.py and the package read no environment variable."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.29e12      # bytes / s


def decode_ms(lib, iq_file, quality, steps, warmup):
    """child process: the segment's decode time through the library `lib`"""
    import numpy as np
    import torch
    import gr_dvbt_amd.binding as b
    if lib:
        b._SO = os.path.abspath(lib)
    iq = np.load(iq_file)
    rx = b.Rx(b.QAM64, b.C7_8, b.T8k, max_samples=len(iq))
    if quality:
        rx.enable_quality()
    dev = torch.from_numpy(iq.view(np.float32)).cuda()
    for _ in range(warmup):
        rx.run_device(dev.data_ptr(), len(iq))
    rx.enable_timing(1)
    for _ in range(steps):                          # (the stage events are read by dvbt_rx_segment_finish: the asynchronous entry)
        rx.enqueue_device(dev.data_ptr(), len(iq))
        rep = rx.finish()
    out = {"total_ms": rx.stage_ms("total"), "viterbi_ms": rx.stage_ms("viterbi"), "symbol_kernel_ms": rx.stage_ms("fft"), "n_ts_bytes": int(rep.n_ts_bytes),
           "rs_fail_words": int(rep.rs_fail_words)}
    rx.close()
    print("RESULT " + json.dumps(out))


def child(lib, iq_file, quality, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib or "", iq_file, str(int(quality)), str(steps), str(warmup)]
    txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        decode_ms(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--superframes", type=int, default=65)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import ctypes as C
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    from oracle import pyoracle as po
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    iq = np.ascontiguousarray(po.stream_slice(c, a.superframes, 77), dtype=np.complex64)
    out = {"workload": f"8k QAM64 7/8, {a.superframes} superframes, clean loopback", "samples": int(len(iq)), "iters": a.iters, "warmup": a.warmup,
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "iq.npy")
        np.save(f, iq)
        out["decode_quality_off"] = child("", f, 0, a.steps, a.warmup)
        out["decode_quality_on"] = child("", f, 1, a.steps, a.warmup)
        out["decode_parent"] = child(a.parent_lib, f, 0, a.steps, a.warmup) if a.parent_lib else None
    L = g.lib()
    L.dvbt_debug_quality_time.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rx = g.Rx(g.QAM64, g.C7_8, g.T8k, max_samples=len(iq), quality=True)
    dev = torch.from_numpy(iq.view(np.float32)).cuda()
    rep = rx.run_device(dev.data_ptr(), len(iq))
    for _ in range(a.warmup):
        q = rx.quality()
    call = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        q = rx.quality()
        call.append((time.perf_counter() - t0) * 1e3)
    ms = np.zeros((4, a.iters), np.float32)
    nbytes = np.zeros(4, np.int64)
    r = L.dvbt_debug_quality_time(rx.h, a.warmup, a.iters, ms.ctypes.data_as(C.c_void_p), nbytes.ctypes.data_as(C.c_void_p))
    assert r == 0, L.dvbt_last_error()
    rx.close()
    out["report"] = {"n_viterbi_bytes": int(rep.n_viterbi_bytes), "n_rs_bytes": int(rep.n_rs_bytes), "n_out_symbols": int(rep.n_out_symbols)}
    out["quality"] = {k: getattr(q, k) for k, _ in g.RxQuality._fields_}
    out["quality"].update(mer_db=q.mer_db, channel_ber=q.channel_ber, post_viterbi_ber=q.post_viterbi_ber)
    out["kernels"] = {}
    for k, name in enumerate(("quality_mer_kernel", "quality_sum_kernel", "quality_channel_kernel", "quality_rs_kernel")):
        med = float(np.median(ms[k]))
        out["kernels"][name] = {"median_ms": med, "min_ms": float(ms[k].min()), "max_ms": float(ms[k].max()), "bytes_read": int(nbytes[k]),
                                "fraction_of_hbm_rate": (float(nbytes[k]) / (med * 1e-3) / HBM_ACHIEVABLE) if med > 0 else None}
    out["kernels_sum_ms"] = float(sum(v["median_ms"] for v in out["kernels"].values()))
    out["quality_call_ms"] = {"median": float(np.median(call)), "min": float(min(call)), "max": float(max(call))}
    base = out["decode_parent"] or None
    out["call_over_parent_decode"] = (out["quality_call_ms"]["median"] / base["total_ms"]) if base else None
    out["decode_on_over_off"] = out["decode_quality_on"]["total_ms"] / out["decode_quality_off"]["total_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
