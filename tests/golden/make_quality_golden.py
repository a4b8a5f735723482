#!/usr/bin/env python3
"""Write tests/golden/quality_ref.json: the figures of the signal-quality model (tests/qualref.py) on the oracle's taps of the
loopback cases of tests/qualcases.py.  Recorded results only; run from the repository root."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as po  # noqa: E402
import qualcases  # noqa: E402
import qualref  # noqa: E402


def figures(c):
    """the model on the oracle's taps of one case, as the fixture records them"""
    cfg, iq = qualcases.make_iq(po, c)
    ref = po.rx(cfg, iq, snr_db=qualcases.rx_snr(c), want=("eq", "demap", "bitdeint", "vit", "deint", "rs"))
    periods = sum(1 for _, n in ref["lock_periods"] if n > 1)
    words = len(ref["rs"]) // 188
    post_bits, post_err = qualref.post_errors(ref["deint"], ref["rs"])
    out = {"periods": periods, "rs_words": words, "rs_fail": int(ref["rs_fail"]), "rs_corr": int(ref["rs_corr"]),
           "post_bits": post_bits, "post_bit_errors": post_err, "n_viterbi_bytes": int(len(ref["vit"]))}
    if periods == 1:
        bits, err = qualref.channel_errors(ref["bitdeint"], ref["vit"], cfg.m, c[2])
        bits6, err6 = qualref.channel_errors(ref["bitdeint"], ref["vit"], cfg.m, c[2], first_step=6)
        out.update(channel_bits_from_step_6=bits6, channel_bit_errors_from_step_6=err6)
        n, sig, e = qualref.mer(ref["eq"], cfg.m, cfg.norm)
        out.update(channel_bits=bits, channel_bit_errors=err, mer_carriers=n, mer_db=round(qualref.mer_db(sig, e), 4))
    return out


def main():
    out = {c[0]: figures(c) for c in qualcases.CASES}
    with open(os.path.join(HERE, "quality_ref.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
