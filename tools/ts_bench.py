"""What the transport-stream analyser costs (dvbt_ts_push_device) on the headline workload's output: 343,980 packets -- the TS of 65 superframes of 8k QAM64
7/8 -- in device memory, pushed in one call; and, in the same session, what dvbt_rf_run_device with every stage off takes over the same number of bytes (a
pass that reads and writes the buffer).

  python tools/ts_bench.py [--out FILE] [--packets 343980] [--iters 20] [--warmup 3] [--what mix|random|rf|all] [--kernel-stats CSV]

Two inputs: `mix`, a realistic multiplex of 30 PIDs (a video PID with a PCR at 56 %, null packets at 10 %, the rest shared, every counter correct), and
`random`, the same packets with uniformly random PIDs -- the worst case for the run lists, close to one run per packet.  As one JSON document: per input the
HIP-event time of the push (median, min, max of --iters calls behind --warmup; the handle is reset before each, outside the timed span), the time per
packet and the ratio to the RF pass; whether the expectation (a ratio of at most 1.0 for `mix`) was met.  --what with one name runs that alone and writes no
file: the form a trace run (rocprofv3 --kernel-trace --stats -- python tools/ts_bench.py --what mix) takes.  --kernel-stats folds the three kernels' times
from such a run's kernel_stats CSV into the document FILE, under the name --what gives, and runs nothing.  Measurement aids live here; bench.py and the
package read no environment variable."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INPUTS = ("mix", "random")
KERNELS = ("ts_parse_kernel", "ts_tile_kernel", "ts_carry_kernel")
TPP = 1282                       # 27 MHz ticks per packet at 31.67 Mbit/s


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


def make_packets(np, kind, n):
    """([n][188] uint8, the PID of every packet)"""
    rs = np.random.RandomState(77)
    pk = rs.randint(0, 256, size=(n, 188), dtype=np.uint8)
    pids = np.array([0x100, 0x1FFF] + [0x101 + k for k in range(20)] + [0x000, 0x010, 0x011, 0x012, 0x014, 0x020, 0x021, 0x030], dtype=np.int64)
    shares = np.array([0.56, 0.10] + [0.30 / 20] * 20 + [0.005] * 8)
    pid = pids[rs.choice(len(pids), size=n, p=shares / shares.sum())]
    cc = np.zeros(n, np.int64)
    for p in pids:
        idx = np.flatnonzero(pid == p)
        cc[idx] = (np.arange(len(idx)) + 1) & 15
    pk[:, 0], pk[:, 3] = 0x47, 0x10 | cc
    video = np.flatnonzero(pid == 0x100)[::40]                             # a PCR on every 40th packet of the video PID: about 3 ms
    pcr = video * TPP + 1000
    base, ext = pcr // 300, pcr % 300
    pk[video, 3] |= 0x20
    pk[video, 4], pk[video, 5] = 7, 0x10
    for k, sh in enumerate((25, 17, 9, 1)):
        pk[video, 6 + k] = (base >> sh) & 255
    pk[video, 10], pk[video, 11] = ((base & 1) << 7) | 0x7e | (ext >> 8), ext & 255
    if kind == "random":
        pid = rs.randint(0, 8192, size=n).astype(np.int64)
    pk[:, 1], pk[:, 2] = pid >> 8, pid & 255
    return pk, pid


def fold_kernel_stats(path, doc_path, name):
    with open(doc_path) as fh:
        doc = json.load(fh)
    rows = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row.get("Name", ""):
                    rows[k] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                               "max_us": float(row["MaxNs"]) / 1e3}
    doc.setdefault("kernels", {})[name] = rows
    with open(doc_path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ts_8k_qam64_7_8_65sf.json"))
    ap.add_argument("--packets", type=int, default=343980)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", choices=INPUTS + ("rf", "all"), default="all")
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        return fold_kernel_stats(a.kernel_stats, a.out, a.what)
    import numpy as np
    import torch
    import gr_dvbt_amd as g
    if g.device_count() <= 0:
        raise SystemExit("ts_bench needs a GPU: libdvbt_hip has no CPU fallback")
    n = a.packets
    nbytes = 188 * n
    samples = nbytes // 8
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    out = {"workload": f"{n} packets of 188 bytes (the TS of 8k QAM64 7/8, 65 superframes), dvbt_ts_push_device in one call",
           "packets": n, "bytes": nbytes, "tile": g.TS_TILE, "iters": a.iters, "warmup": a.warmup}
    for kind in INPUTS:
        if a.what not in (kind, "all"):
            continue
        pk, pid = make_packets(np, kind, n)
        x = torch.from_numpy(pk).to(dev)
        torch.cuda.synchronize()
        t = g.TsAnalyser(max_packets=n)

        def before():
            t.reset()
            torch.cuda.synchronize()
        ms = timed(stream, a.iters, a.warmup, before, lambda: t.push_device(x.data_ptr(), n, stream=stream.cuda_stream))
        r = t.read()
        t.close()
        count = np.bincount(pid, minlength=8192)
        seen = np.flatnonzero(count)
        assert r.packets_pushed == n and r.sync_errors == 0 and np.array_equal(r.pids["pid"], seen) and np.array_equal(r.pids["packets"], count[seen])
        med = float(np.median(ms))
        out[kind] = {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "ns_per_packet": med * 1e6 / n, "pids_seen": r.pids_seen,
                     "cc_errors": int(r.pids["cc_errors"].sum()), "pcr_pairs": int(r.pids["pcr_pairs"].sum())}
        if kind == "mix":
            assert out[kind]["cc_errors"] == 0 and abs(r.ts_bitrate(0x100) - 188 * 8 * 27e6 / TPP) < 1e-6 * r.ts_bitrate(0x100)
            out[kind]["ts_bitrate"] = r.ts_bitrate(0x100)
        del x
    if a.what in ("rf", "all"):
        x = torch.zeros(2 * samples, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        rf = g.RfFrontend()                                                # every stage off: the pass reads and writes the buffer
        ms = timed(stream, a.iters, a.warmup, lambda: None, lambda: rf.run_device(x.data_ptr(), samples, y.data_ptr(), stream=stream.cuda_stream))
        rf.close()
        med = float(np.median(ms))
        out["rf_all_off"] = {"samples": samples, "median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms))}
    if a.what == "all":
        for kind in INPUTS:
            out[kind]["over_rf_all_off"] = out[kind]["median_ms"] / out["rf_all_off"]["median_ms"]
        out["expectation"] = {"what": "mix over rf_all_off at most 1.0", "met": bool(out["mix"]["over_rf_all_off"] <= 1.0)}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
