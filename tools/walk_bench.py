"""bench.py with the Viterbi decoder's shortcut switched off (dvbt_rx_set_viterbi_walk(h, 1) on every handle bench.py creates): what the decision in front of the windows
costs where it never pays.  `python tools/walk_bench.py <bench args>` on the GPU box; with `--counters` in front of the bench arguments the shortcut stays ON and the handles'
counters (shortcut / walked iterations, summed over every handle that was created, the pre-scan's and the warm-up steps' included) are written as one JSON line to stderr.
Measurement aids live here; bench.py and the package read no environment variable."""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
args = sys.argv[1:]
counters = "--counters" in args
args = [a for a in args if a != "--counters"]
import torch  # noqa: F401,E402
import gr_dvbt_amd as g  # noqa: E402
import gr_dvbt_amd.binding as b  # noqa: E402

total = [0, 0]
live = []


def _count(rx):
    try:
        s, w = rx.viterbi_shortcut()
        total[0] += s
        total[1] += w
    except RuntimeError:
        pass                                                       # (a handle without the proof: no counters)


class Rx(b.Rx):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        if counters:
            live.append(self)
        else:
            self.set_viterbi_walk(1)

    def close(self):
        if self.h and self in live:
            live.remove(self)
            _count(self)
        super().close()


b.Rx = g.Rx = Rx
import bench  # noqa: E402
sys.argv = ["bench.py"] + args
bench.main()
if counters:
    for rx in list(live):
        if rx.h:
            _count(rx)
    os.write(2, (json.dumps({"viterbi_shortcut_iterations": total[0], "viterbi_walked_iterations": total[1]}) + "\n").encode())   # (bench.py keeps stdout for its own line)
