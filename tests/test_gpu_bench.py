"""bench.py's plain run and --dump-outputs: the plain result line carries the headline alone, and the dump of the last timed step is the same
from run to run -- the TS that --full verifies against the transmitted packets."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "3", "--warmup", "1", "--superframes", "4"]
DUMPED = ("ts_packet_checksum", "ts_sample", "ts_sample_index", "piece_meta")


def _bench(*args):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=e, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_verified_ts(tmp_path):
    d = _bench(*SMALL, "--dump-outputs", str(tmp_path / "plain"))
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Msamples/s" and d["higher_is_better"] is True
    assert abs(d["ms_per_step"] * 3 - d["timed_region_s"] * 1e3) < 0.01 * d["timed_region_s"] * 1e3 + 1.0      # timed_region_s is rounded to the ms
    assert "cpu_baseline" not in d and "extra_workloads" not in d and "verified" not in d["config"] and d["stage_ms_per_piece_solo"] is None
    f = _bench(*SMALL, "--full", "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(tmp_path / "full"))
    c = f["config"]
    assert c["verified"] is True and c["wrong_bytes"] == 0 and f["stage_ms_per_piece_solo"] is not None
    total = 0
    for name in DUMPED:
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    chk = np.load(tmp_path / "plain" / "ts_packet_checksum.npy")
    idx = np.load(tmp_path / "plain" / "ts_sample_index.npy")
    assert len(chk) == c["ts_packets"] > 0 and 0 <= idx.min() and idx.max() < c["ts_bytes"] == d["config"]["ts_bytes_per_step"]
