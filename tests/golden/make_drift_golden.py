#!/usr/bin/env python3
"""Write tests/golden/drift_eps_8k_echo_cfo.txt: the oracle's epsilon (ofdm_sym_acquisition's fractional carrier-offset estimate, one value per call) over its
lock period on 8k QAM64 7/8, 2 superframes, stream seed 9, an echo at 77 samples of amplitude 0.1 and a carrier offset of 0.003 subcarriers -- the "8k echo 0.3 cp
-20 dB + cfo 0.003" case of tests/test_gpu_channel.py.  An offset that small with estimates that jitter is where the increments of the float phase accumulator are a
few of its ulps (tests/test_drift_model.py, tests/test_gpu_drift_kernels.py).  Recorded results only, one float32 per line; run from the repository root."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402


def main():
    c = po.cfg(po.QAM64, po.C7_8, po.T8k)
    iq = po.channel(po.stream_slice(c, 2, 9), c.N, echoes=((77, 0.1),), cfo=0.003)
    o = po.rx(c, iq, want=("ts",))
    assert o["truncated"] == 0 and o["first_out_symbol"] >= 0, "the case is meant to hold the lock"
    eps = np.asarray(o["epsilon"], dtype=np.float32)[:o["n_acquired"]]
    with open(os.path.join(HERE, "drift_eps_8k_echo_cfo.txt"), "w") as f:
        for e in eps:
            f.write(repr(float(e)) + "\n")
    print(f"{len(eps)} calls, first output symbol {o['first_out_symbol']}, epsilon {eps.min():.4f} .. {eps.max():.4f}, mean {eps.mean():.4f}, std {eps.std():.2e}")


if __name__ == "__main__":
    main()
