"""The corpora of tests/rxref.py for the segment chain's outer stage (tests/test_gpu_outer.py), on the references alone: every named case is what it
claims to be -- the bad words of every wavefront, the words the defer list will hold, the four kinds of sync-byte patch on packets the descrambler
examines, the runs of the descrambler.  No GPU: what is checked here is the test's input, not the kernels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rxref  # noqa: E402
from rxref import JUNCTION, NSYNC, WAVE  # noqa: E402


def _ref(po, name, compat=0):
    c = rxref.outer_case(po, name)
    return c, rxref.outer_reference(po, c["stream"], compat)


def test_output_word_w_is_corpus_word_w_minus_11_and_the_junction_words_fail(po):
    for name in ("clean-80", "load-25", "phase-5"):
        c, r = _ref(po, name)
        n = r["n_words"]
        assert n == rxref.segment_words(len(c["stream"])) == c["n_out"]
        assert (r["deint"][JUNCTION:] == c["corpus"][:n - JUNCTION]).all()
        assert (r["deint"][:JUNCTION, 0] == 0).all()
    # the 11 junction words of a clean stream are what fails, and nothing else is touched
    for n_out in rxref.CLEAN_SIZES:
        c, r = _ref(po, f"clean-{n_out}")
        assert (r["n_words"], r["fail"], r["corr"]) == (n_out, JUNCTION, 0)
        assert (r["rs"][JUNCTION:] == c["corpus"][:n_out - JUNCTION, :188]).all()
        assert rxref.deferred_words(rxref.bad_per_wave(c["nerr"], n_out)) == JUNCTION
        assert len(rxref.descramble_runs(r["rs"])[0]) == (1 if n_out >= 48 else 0)


@pytest.mark.parametrize("load", rxref.LOADS)
def test_load_cases_hold_the_bad_words_they_claim(po, load):
    c, r = _ref(po, f"load-{load}")
    bad = rxref.bad_per_wave(c["nerr"], c["n_out"])
    assert len(bad) == 25
    assert bad[0] == min(load + JUNCTION, WAVE) and (bad[1:24] == load).all() and bad[24] == min(load, 16)
    paths = [rxref.rs_path(b) for b in bad]
    if load in (12, 13):                                       # wavefront 0 stands on either side of the switch, the others stay on the defer list
        assert paths[0] == ("wave" if load == 12 else "lane") and set(paths[1:]) == {"wave"}
    want = sum(b for b in bad if b < rxref.RS_LANE_MIN)
    assert rxref.deferred_words(bad) == want
    if load == 23:
        assert want == 23 * 23 + 16 > 512                       # the second trip of rs_fix_kernel's 512 workgroups
    # errors of every size, garbage words, and the decoder's verdict: a word with 8 errors or fewer comes back as it was sent
    ne = c["nerr"][:c["n_out"] - JUNCTION]
    assert set(ne[ne > 0]) == set(range(1, 17)) and (ne == -1).sum() >= 2
    ok = (ne >= 0) & (ne <= 8)
    assert (r["rs"][JUNCTION:][ok] == c["sent"][:len(ne), :188][ok]).all()
    assert r["fail"] >= JUNCTION + (ne > 8).sum()


def test_cycle_and_range_cases_mix_both_decoders_in_one_launch(po):
    for name, waves in (("cycle", 25), ("range", 32)):
        c, _ = _ref(po, name)
        bad = rxref.bad_per_wave(c["nerr"], c["n_out"])
        assert len(bad) == waves
        whole = c["n_out"] // WAVE
        assert list(bad[:whole]) == [rxref.CYCLE[w % 4] for w in range(whole)]
        assert {rxref.rs_path(b) for b in bad} == {"none", "wave", "lane"}
        assert 0 < rxref.deferred_words(bad) < 512


def test_phase_cases_lock_in_the_first_window_or_drop_two_items_first(po):
    first_window, dropped = 0, 0
    for p in range(8):
        c, r = _ref(po, f"phase-{p}")
        runs, _, ts = rxref.descramble_runs(r["rs"])
        first = min(w for w in range(JUNCTION, 32) if w % 8 == p)
        assert len(runs) == 1 and runs[0][0] == first
        assert len(ts) == len(r["ts"]) and (ts == r["ts"]).all()
        first_window += first < 16
        dropped += first >= 16
    assert first_window == 5 and dropped == 3


def test_kinds_case_has_eight_words_of_every_kind_on_examined_packets(po):
    c, r = _ref(po, "kinds")
    n = r["n_words"]
    runs, looked, ts = rxref.descramble_runs(r["rs"])
    assert (ts == r["ts"]).all() and len(runs) == 5                 # four breaks
    bad = rxref.bad_per_wave(c["nerr"], n)
    deferred_wave = np.repeat((bad > 0) & (bad < rxref.RS_LANE_MIN), WAVE)[:n]
    lane_wave = np.repeat(bad >= rxref.RS_LANE_MIN, WAVE)[:n]
    seen = np.zeros(n, bool)
    seen[looked] = True
    got, sent = r["deint"][:, 0] == NSYNC, r["rs"][:, 0] == NSYNC
    for kind, mask in (("restored", ~got & sent), ("removed", got & ~sent)):
        for where, wave in (("deferred", deferred_wave), ("lane", lane_wave)):
            assert (mask & wave & seen).sum() >= 8, (kind, where, (mask & wave & seen).sum())
    # every break is an uncorrectable word on the call grid
    for src, _ in runs[1:]:
        at = max(w for w in looked if w < src and r["rs"][w, 0] != NSYNC and w % 8 == 0)
        assert c["nerr"][at - JUNCTION] == -1
    # rs_oracle_compat = 1 leaves the lowest error of a word where it is (the reference's omega[2t] overflow): no sync byte is patched, every one of
    # the corpus's sync errors is then a break or a false lock of the descrambler -- the bytes still have one right answer
    r1 = rxref.outer_reference(po, c["stream"], 1)
    runs1, _, ts1 = rxref.descramble_runs(r1["rs"])
    assert ((r1["deint"][:, 0] == NSYNC) == (r1["rs"][:, 0] == NSYNC)).all()
    assert len(runs1) > len(runs) and (ts1 == r1["ts"]).all()


def test_lost_sync_and_jump_cases(po):
    c, r = _ref(po, "nosync")
    sync = r["rs"][:, 0] == NSYNC
    gaps = np.diff(np.flatnonzero(sync))
    assert gaps.max() >= 40 + 8                                     # packets from one NSYNC to the next: 48 and more without
    runs, _, _ = rxref.descramble_runs(r["rs"])
    assert len(runs) == 2
    phases = set()
    for k in range(1, 15):
        c, r = _ref(po, f"jump-{k}")
        runs, _, ts = rxref.descramble_runs(r["rs"])
        assert (ts == r["ts"]).all()
        assert len(runs) == (1 if k == 8 else 2), (k, runs)         # eight words missing: the NSYNC stays where the descrambler looks
        phases.add(runs[-1][0] % 8)
    assert len(phases) == 8
    c, r = _ref(po, "both")
    runs, _, ts = rxref.descramble_runs(r["rs"])
    assert len(runs) == 3 and (ts == r["ts"]).all()


def test_runs_case_exceeds_the_old_run_list(po):
    c, r = _ref(po, "runs")
    assert c["n_out"] < 60000
    runs, _, ts = rxref.descramble_runs(r["rs"])
    assert len(runs) > rxref.DESCR_MAX_RUNS
    assert np.median([n for _, n in runs]) == 48                    # three calls per run
    assert len(ts) == len(r["ts"]) == sum(n for _, n in runs) * 188 and (ts == r["ts"]).all()


def test_long_case_breaks_behind_call_8192(po):
    c, r = _ref(po, "long")
    assert c["n_out"] >= 131200
    runs, _, ts = rxref.descramble_runs(r["rs"])
    assert runs == [(16, 16 * rxref.LONG_BREAK_CALL), (16 + 16 * rxref.LONG_BREAK_CALL + 8, 176)]
    assert rxref.LONG_BREAK_CALL > 8192
    assert len(ts) == len(r["ts"]) and (ts == r["ts"]).all()


def test_cut_reference_follows_the_contract(po):
    """clean pieces: every phase's call positions carry their NSYNC; the piece delivers from its first NSYNC in whole groups"""
    L = rxref._outer_lib(po)
    for p in range(16):
        c = rxref.outer_case(po, f"cut-{p % 8}")
        for n in (11, 12, 27, 43, 44, 700):
            r = rxref.outer_reference(po, c["stream"], 0, n_words=n, descramble=False)
            q, ts, unclean = rxref.cut_reference(po, r["rs"], p)
            first = min(w for w in range(JUNCTION, 32) if w % 8 == p % 8)
            assert unclean == 0
            if first < n:
                assert q == first and len(ts) == (n - first) // 8 * 1504
            else:
                assert (q, len(ts)) == (0, 0)
        # a call position of the phase inside [11, n - 32] hit: unclean; only one outside: not
        inside = min(w for w in range(200, 232) if w % 16 == p)
        outside = max(w for w in range(700) if w % 16 == p)
        assert outside + 32 > 700
        for at, want in ((inside, 1), (outside, 0)):
            s = rxref.cut_hit(po, p, at)
            r = rxref.outer_reference(po, s, 0, n_words=700, descramble=False)
            assert r["rs"][at, 0] != NSYNC
            assert rxref.cut_reference(po, r["rs"], p)[2] == want
    assert L is not None


def test_bitmap_reference():
    rs = np.zeros((70, 188), np.uint8)
    rs[[0, 5, 63, 64, 69], 0] = NSYNC
    bm = rxref.sync_bitmap(rs, 70)
    assert list(bm) == [(1 << 0) | (1 << 5) | (1 << 63), (1 << 0) | (1 << 5)]
    assert list(rxref.sync_bitmap(rs, 69)) == [(1 << 0) | (1 << 5) | (1 << 63), 1]
