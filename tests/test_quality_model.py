"""tests/qualref.py, the model of the blind signal-quality figures, pinned: on the oracle's taps of five seeded loopbacks against recorded
results (tests/golden/quality_ref.json, written by tests/golden/make_quality_golden.py), and against itself (what it encodes has no errors,
what is flipped is counted once)."""
import json
import os

import numpy as np
import pytest

import qualcases
import qualref
from oracle import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))

# The figures the feature's specification states for these cases: (channel errors, channel bits, post errors, RS words, rs_fail, rs_corr, periods, MER dB).
# Its channel counts were taken from step 6 on (the first step with six predecessors); the counted set it defines, and the kernels count,
# starts at step 8 (the first whole decoded byte behind them).  Both are pinned: the stated numbers with first_step = 6, the fixture's with 8.
STATED = {
    "2k_qam16_1_2_4sf_clean": (0, 4928932, 0, 1504, 11, 0, 1, None),
    "2k_qam16_1_2_4sf_12dB": (197006, 4928932, 1942, 1504, 11, 787, 1, 11.75),
    "2k_qam64_7_8_4sf_24dB": (4754, 7397150, 399, 3952, 11, 125, 1, 23.02),
    "8k_qam64_3_4_1sf_19dB": (58802, 2466702, 9981, 1120, 652, 3031, 1, 18.89),
    "2k_qam16_1_2_4sf_9dB": (None, None, None, 1296, 1296, 0, 4, None),
}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "quality_ref.json")) as f:
        return json.load(f)


_taps = {}


def taps(name):
    """the oracle's taps of a case (computed once per run)"""
    if name not in _taps:
        c = qualcases.case(name)
        cfg, iq = qualcases.make_iq(po, c)
        ref = po.rx(cfg, iq, snr_db=qualcases.rx_snr(c), want=("eq", "demap", "bitdeint", "vit", "deint", "rs"))
        _taps[name] = (c, cfg.m, float(cfg.norm), ref)
    return _taps[name]


@pytest.mark.parametrize("name", [c[0] for c in qualcases.CASES])
def test_model_on_the_oracles_taps(name, golden):
    c, m, norm, ref = taps(name)
    g = golden[name]
    st = STATED[name]
    periods = sum(1 for _, n in ref["lock_periods"] if n > 1)
    words = len(ref["rs"]) // 188
    assert (periods, words, int(ref["rs_fail"]), int(ref["rs_corr"])) == (g["periods"], g["rs_words"], g["rs_fail"], g["rs_corr"]) == (st[6], st[3], st[4], st[5])
    assert len(ref["vit"]) == g["n_viterbi_bytes"]
    # the byte de-interleaver in closed form is the oracle's, from the first byte of the segment's Viterbi stream
    assert len(ref["deint"]) == 204 * words
    assert np.array_equal(qualref.deint_from_viterbi(ref["vit"], words), ref["deint"])
    post = qualref.post_errors(ref["deint"], ref["rs"])
    assert post == (g["post_bits"], g["post_bit_errors"]) and post[0] == 1504 * words
    if st[2] is not None:
        assert post[1] == st[2]
    if periods != 1:
        assert "channel_bits" not in g and "mer_db" not in g
        return
    inp = ref["bitdeint"]
    assert qualref.channel_errors(inp, ref["vit"], m, c[2]) == (g["channel_bits"], g["channel_bit_errors"])
    from6 = qualref.channel_errors(inp, ref["vit"], m, c[2], first_step=6)
    assert from6 == (g["channel_bits_from_step_6"], g["channel_bit_errors_from_step_6"]) == (st[1], st[0])
    n, sig, err = qualref.mer(ref["eq"], m, norm)
    assert n == g["mer_carriers"] == ref["eq"].size
    db = qualref.mer_db(sig, err)
    print(name, "MER", db, "dB")
    assert abs(db - g["mer_db"]) <= 0.01
    if st[7] is None:
        assert db > 60.0
    else:
        assert abs(db - st[7]) <= 0.01
    # the nearest grid point is the point of the demapper's label: every label goes with one grid cell, every cell with one label
    L = 1 << (m // 2)
    lab = np.asarray(ref["demap"]).reshape(-1).astype(np.int64)
    eq = ref["eq"].reshape(-1)
    step = 2.0 * float(np.float32(norm))
    i_re = np.clip(np.floor(eq.real.astype(np.float64) / step + L / 2.0), 0, L - 1).astype(np.int64)
    i_im = np.clip(np.floor(eq.imag.astype(np.float64) / step + L / 2.0), 0, L - 1).astype(np.int64)
    pairs = np.unique(lab * 64 + i_re * L + i_im)
    assert len(pairs) == len(np.unique(pairs // 64)) == len(np.unique(pairs % 64)) == len(np.unique(lab))


@pytest.mark.parametrize("m", [2, 4, 6])
@pytest.mark.parametrize("code_rate", [0, 1, 2, 3, 4])
def test_model_counts_what_is_flipped(code_rate, m):
    rng = np.random.RandomState(100 + 10 * code_rate + m)
    n_vit = 997
    vit = rng.randint(0, 256, n_vit).astype(np.uint8)
    bits = qualref.info_bits(vit)
    # the input covers a little more than the decoded bytes, as the chain's does (the decoder lags by its traceback depth)
    tail = rng.randint(0, 2, 8 * 30).astype(np.uint8)
    inp = qualref.puncture_pack(np.concatenate([bits, tail]), code_rate, m)
    total, err = qualref.channel_errors(inp, vit, m, code_rate)
    q, _ = qualref.counted_set(n_vit, len(inp), m, code_rate)
    assert err == 0 and total == len(q) > 0
    k = qualref.RATE_K[code_rate]
    assert total == len(qualref.kept_positions(8 * n_vit, code_rate)) - len(qualref.kept_positions(8, code_rate))
    assert abs(total - (8 * n_vit - 8) * (k + 1) / k) < 2
    K = 50
    flips = rng.choice(len(inp) * m, K, replace=False)
    flips[0] = 0                                        # one in front of the counted set
    flips = np.unique(flips)
    bad = inp.copy()
    for f in flips:
        bad[f // m] ^= 1 << (m - 1 - f % m)
    inside = np.isin(flips, q).sum()
    assert 0 < inside < len(flips)
    assert qualref.channel_errors(bad, vit, m, code_rate) == (total, int(inside))
    # a short input clips the counted set
    short = inp[:len(inp) // 2]
    qs, _ = qualref.counted_set(n_vit, len(short), m, code_rate)
    assert qualref.channel_errors(short, vit, m, code_rate) == (len(qs), 0) and 0 < len(qs) < total
