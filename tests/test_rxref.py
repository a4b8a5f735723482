"""The references of tests/rxref.py against the oracle (CPU only): the receive-block sweep rests on them.

The RS corpus must hold what it is asked for (bad words per wavefront, error counts and places) and decode with the oracle back to its payloads
wherever the code can; the call-by-call energy_descramble restatement must deliver the oracle's o_energy_descramble bytes on a clean stream for
every group-start offset and any call sizes, and follow a lost or slipped sync the way the reference's general_work does.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rxref  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _oracle_rs(po, words, compat):
    rs = po.RS()
    po.lib().o_rs_init(C.byref(rs))
    out = np.zeros((len(words), 188), np.uint8)
    nf, nc = C.c_int(), C.c_int()
    po.lib().o_rs_dec_block(C.byref(rs), _p(words), _p(out), C.c_size_t(len(words)), compat, C.byref(nf), C.byref(nc))
    return out, nf.value, nc.value


@pytest.mark.parametrize("bad", [0, 1, 23, 24, 63, 64])
@pytest.mark.parametrize("where", ["random", "first", "last", "burst", "parity"])
def test_rs_corpus(po, bad, where):
    nwords = 64 * 3 + 37                                                 # a partial last wavefront
    errs = (1, 2, 8, 3, 16, 5, 9, 7, 4, 8) if where != "burst" else (8, 1, 8, 5, 8, 2)
    cor = rxref.rs_corpus(po, nwords, bad, errors=errs, where=where, garbage_every=7 if bad > 1 else 0, seed=bad)
    w, nerr = cor["words"], cor["nerr"]
    assert list(cor["bad_per_wave"]) == [min(bad, 64)] * 3 + [min(bad, 37)]
    assert [rxref.rs_path(b) for b in cor["bad_per_wave"]][0] == ("none" if bad == 0 else "wave" if bad < 24 else "lane")
    # the error counts are exact: a word differs from its codeword in nerr bytes
    clean = rxref.rs_corpus(po, nwords, 0, seed=bad)["words"]
    diff = (w != clean).sum(axis=1)
    assert ((diff == nerr) | (nerr < 0)).all()
    assert (cor["payload"] == clean[:, :188]).all()
    sel = nerr > 0
    if where == "first":
        assert (w[sel, 0] != clean[sel, 0]).all()
    elif where == "last":
        assert (w[sel, 203] != clean[sel, 203]).all()
    elif where == "parity":
        assert (w[sel, :188] == clean[sel, :188]).all()
    elif where == "burst":
        for i in np.flatnonzero(sel):
            d = np.flatnonzero(w[i] != clean[i])
            assert d[-1] - d[0] + 1 == nerr[i]
    # the oracle (compat = 0) returns the payload of every word with at most 8 errors
    out, nf, nc = _oracle_rs(po, w, 0)
    ok = (nerr >= 0) & (nerr <= 8)
    assert (out[ok] == cor["payload"][ok]).all()
    assert nf >= ((nerr > 8) | (nerr < 0)).sum() - 2 or bad == 0        # (a word beyond t is almost never miscorrected into a codeword)
    assert nc == nerr[(nerr > 0) & (nerr <= 8)].sum()


def _dispersed(po, npackets, seed):
    ts = po.make_ts(npackets, seed)
    disp = np.zeros_like(ts)
    po.lib().o_energy_dispersal(_p(ts), _p(disp), C.c_size_t(npackets))
    return ts, disp


def test_prbs_group_is_the_oracles(po):
    seq = np.zeros(1504, np.uint8)
    po.lib().o_energy_prbs(_p(seq))
    assert (rxref.prbs_group() == seq).all()


@pytest.mark.parametrize("offset", range(16))
def test_descramble_calls_is_the_oracle_on_a_clean_stream(po, offset):
    """the first group starts `offset` packets into the stream (junk packets with an ordinary sync byte in front); the oracle runs the rule in
    the smallest calls, the restatement in calls of mixed sizes: the same bytes up to where the larger calls stop"""
    rng = np.random.RandomState(offset)
    ts, disp = _dispersed(po, 8 * 80, offset)
    junk = rng.randint(0, 256, (offset, 188)).astype(np.uint8)
    junk[:, 0] = rxref.SYNC
    x = np.concatenate([junk.reshape(-1), disp])
    x = x[:len(x) // 1504 * 1504]
    nitems = len(x) // 1504
    ref = np.zeros(len(x), np.uint8)
    n_ref = po.lib().o_energy_descramble(_p(x), C.c_size_t(nitems), _p(ref))
    for calls in ([4] * 40, [8, 4, 12, 64, 4, 8], [64], [12] * 5):
        res, d_index = rxref.descramble_calls(x, calls)
        out = np.concatenate([r[2] for r in res])
        assert all(r[1] == r[0] * 1504 and r[1] > 0 for r in res)            # locked from the first call: nothing dropped
        assert d_index == offset * 188                                       # found in the first call, kept: the NSYNC recurs there
        assert 0 < len(out) <= n_ref and (out == ref[:len(out)]).all()
        # and it is the transmitted TS from the first NSYNC packet on
        assert (out == ts[:len(out)]).all()


def test_descramble_calls_lost_and_slipped_sync(po):
    """a stretch without any NSYNC drops two items per call and sends the search back to offset 0; a one-packet slip moves the lock to the next
    NSYNC at or after the carried offset (not the earliest one of the window)"""
    ts, disp = _dispersed(po, 8 * 60, 5)
    x = disp[3 * 188:].copy()                                             # NSYNC at packet 5 of every item
    x = x[:len(x) // 1504 * 1504]
    dead = x.copy()
    dead[20 * 1504:26 * 1504:188] = rxref.SYNC                            # items 20..25: every sync byte ordinary
    res, d_index = rxref.descramble_calls(dead, [4] * 30)
    drops = [i for i, r in enumerate(res) if r[1] == 0]
    assert drops and all(r[0] == 2 for i, r in enumerate(res) if i in drops)
    assert d_index == 5 * 188
    slip = np.concatenate([x[:30 * 1504 + 188 * 6], x[30 * 1504 + 188 * 7:]])     # one packet (not a sync one) removed inside item 30
    slip = slip[:len(slip) // 1504 * 1504]
    res, d_index = rxref.descramble_calls(slip, [4] * 40)
    assert all(r[1] > 0 for r in res)
    assert d_index == 4 * 188 + 8 * 188                                   # searched on from 5 * 188: the next NSYNC, a whole group later
    res0, _ = rxref.descramble_calls(slip, [4] * 40, d_index=0)
    assert len(res0) == len(res)
