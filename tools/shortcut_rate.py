"""How often the Viterbi decoder's traceback takes the shortcut over chained best states (k_viterbi3.hpp) on noisy input, and what the stage costs there: 8k QAM64 7/8, a few
superframes through the segment API, AWGN at 18, 20, 22, 25, 30 dB and clean.  Per noise level one JSON line: the share of iterations (blocks of 24 windows, per wavefront) on the
shortcut, the decoder stage's time (HIP events around it, one step in flight, mean of the timed segments) with the shortcut and with it switched off (dvbt_rx_set_viterbi_walk),
and the RS counters.
`python tools/shortcut_rate.py [superframes=9] > profiles/r09_shortcut_rate.jsonl` on the GPU box."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from oracle import pyoracle as po
import gr_dvbt_amd as g

nsf = int(sys.argv[1]) if len(sys.argv) > 1 else 9
RUNS = 10
c = po.cfg(g.QAM64, g.C7_8, g.T8k)
clean = po.stream_slice(c, nsf, 21)
for snr in (None, 30.0, 25.0, 22.0, 20.0, 18.0):
    iq = po.channel(clean, c.N, seed=5, snr_db=snr) if snr is not None else clean
    dev = torch.from_numpy(iq.view(np.float32)).cuda()
    torch.cuda.synchronize()
    line = {"case": "clean" if snr is None else f"awgn {snr:g} dB", "superframes": nsf, "samples": int(len(iq))}
    for walk in (0, 1):
        rx = g.Rx(g.QAM64, g.C7_8, g.T8k, max_samples=len(iq), snr_db=snr if snr is not None else 30.0)
        rx.set_viterbi_walk(walk)
        rep = rx.run_device(dev.data_ptr(), len(iq))               # (the first run: start-up transients)
        s0, w0 = rx.viterbi_shortcut()
        rx.enable_timing(True)                                     # a new measurement window
        for _ in range(RUNS):
            rx.enqueue_device(dev.data_ptr(), len(iq))
            rep = rx.finish()
        s1, w1 = rx.viterbi_shortcut()
        ms = rx.stage_ms("viterbi")
        if walk == 0:
            it = (s1 - s0) + (w1 - w0)
            line.update({"shortcut_iterations": (s1 - s0) // RUNS, "walked_iterations": (w1 - w0) // RUNS, "shortcut_share": round((s1 - s0) / it, 4) if it else None,
                         "viterbi_ms": round(ms, 4), "lock_periods": int(rep.n_lock_periods), "rs_corrected": int(rep.rs_corrected_symbols),
                         "rs_fail_words": int(rep.rs_fail_words), "ts_bytes": int(rep.n_ts_bytes)})
        else:
            line["viterbi_ms_walk_always"] = round(ms, 4)
        rx.close()
    print(json.dumps(line), flush=True)
