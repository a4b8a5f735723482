"""The layers that cut one stream into pieces and put the bytes back together -- dvbt_rx_set_cut with multi.plan_cuts / stitch_ts, the streaming entry
dvbt_rx_stream_* (csrc/dvbt_stream.inc) and its sharded form -- at every guard interval other than 1/32, all five code rates and 12 of the 15
(constellation, rate) pairs (tests/streamcases.py).  What moves with them: L = N + cp sets every sample offset of the plan (begin, end, launch_at, thr,
len0, cap, win, auto_need); the post-roll runs from 8 symbols to 90 (QPSK 1/2: longer than the pre-roll of 76); the decoded bits per symbol and the packets
per superframe drive the descrambler's call grid and the chunk labels; and the call sizes straddle one slot of the pinned staging ring (131,072 samples) and
the direct-copy threshold (262,144 samples), which a call of a few symbols at L = 2112 / 8448 never does.

Every comparison is byte for byte.  The reference bytes are the ORACLE's chain over the whole stream (streamcases.stream); the HIP single chain is required
to equal them first (single_chain), so no case compares the HIP path with itself alone."""
import time

import numpy as np
import pytest
import torch

import gr_dvbt_amd as g
from gr_dvbt_amd import multi

import streamcases
from streamcases import CELLS, cell, cell_id

pytestmark = pytest.mark.gpu

PIN_SLOT = 131072            # samples in one slot of the pinned staging ring (STREAM_PIN_BYTES / 8)
DIRECT = 262144              # samples from which a host push is copied straight out of the caller's buffer (STREAM_DIRECT_BYTES / 8)


def call_sizes(L):
    return [4 * L, 33 * L + 5, PIN_SLOT - 1, PIN_SLOT + 1, DIRECT - 1, DIRECT]


def call_size(k):
    """cells 1..6 (2k) and 7..12 (8k) go through the list once each: every size meets a 2k and an 8k cell"""
    return call_sizes(k.L)[(k.no - 1) % 6]


def hip_single_chain(const, cr, mode, guard, iq):
    rx = g.Rx(const, cr, mode, max_samples=len(iq), guard=guard)
    rep = rx.run(iq)
    ts = rx.tap(g.TAP_TS).copy()
    rx.close()
    return rep, ts


_single = {}


def single_chain(po, k, nsf=None):
    """(samples, the oracle's TS, the HIP single chain's report) of the cell's stream; the HIP single chain must deliver the oracle's bytes (checked once per stream)"""
    iq, ref = streamcases.stream(po, k, nsf)
    key = (k.no, len(iq))
    if key not in _single:
        rep, ts = hip_single_chain(k.const, k.cr, k.mode, k.guard, iq)
        assert rep.status in (0, 2) and rep.segment_offset == 0                 # 2: the lock ends with the signal (zero tail)
        assert len(ts) == len(ref) > 0 and (ts == ref).all(), "HIP single chain differs from the oracle"
        _single[key] = rep
    return iq, ref, _single[key]


def on_device(iq):
    dev = torch.from_numpy(iq.view(np.float32).copy()).cuda()
    torch.cuda.synchronize()
    return dev


def run_stream(st, iq, call, device=False, pull_every=7):
    """push `iq` in calls of `call` samples (from one resident device buffer if `device`), pull after every pull_every-th push; returns the TS, the info, the
    highest pieces_in_flight seen behind a push, the trace and samples_released behind every push; closes the stream"""
    dev = on_device(iq) if device else None
    out, in_flight, released, k = [], 0, [], 0
    for a in range(0, len(iq), call):
        n = min(call, len(iq) - a)
        if device:
            st.push_device(dev.data_ptr() + 8 * a, n)
        else:
            st.push(iq[a:a + n])
        k += 1
        i = st.info()
        in_flight = max(in_flight, i.pieces_in_flight)
        released.append(i.samples_released)
        if k % pull_every == 0:
            out.append(st.pull())
    st.finish()
    out.append(st.pull())
    info, trace = st.info(), st.trace()
    st.close()
    return np.concatenate(out), info, in_flight, trace, released


def pieces_decoded_the_body(in_flight, trace):
    """the stream reached pieces and stayed there: one epoch, no piece left it (else the walk, not the plan, would have decoded the stream)"""
    lines = trace.splitlines()
    assert in_flight >= 1, trace
    assert sum(1 for ln in lines if ln.startswith("epoch:")) == 1, trace
    assert not any("leaves the epoch" in ln for ln in lines), trace


# ---- (a) cut pieces on separate handles and HIP streams

def decode_pieces(k, iq, cuts):
    """every piece on its own handle and stream; enqueue all, then collect"""
    dev = on_device(iq)
    rxs, streams = [], []
    for cu in cuts:
        rx = g.Rx(k.const, k.cr, k.mode, max_samples=cu["end"] - cu["begin"], guard=k.guard)
        rx.set_cut(cu["sym_off"])
        st = torch.cuda.Stream()
        rx.enqueue_device(dev.data_ptr() + 8 * cu["begin"], cu["end"] - cu["begin"], st.cuda_stream)
        rxs.append(rx); streams.append(st)
    out = [(rx.finish(), rx.tap(g.TAP_TS)) for rx in rxs]
    for rx in rxs:
        rx.close()
    return out


@pytest.mark.parametrize("k", CELLS, ids=cell_id)
def test_stitched_pieces_equal_the_single_segment(po, k):
    nsf, parts = streamcases.cut_size(k)
    d = g.get_dims(k.const, k.cr, k.mode, k.guard)
    assert (d.fft_length + d.cp_length, multi.post_symbols(d)) == (k.L, k.post)
    iq, ref, rep = single_chain(po, k, nsf)
    sf_call = rep.first_call + rep.first_out_symbol
    assert rep.first_out_symbol == streamcases.first_superframe_symbol(k.const, k.mode)
    cuts = multi.plan_cuts(d, len(iq), int(rep.segment_offset), sf_call, parts)
    assert len(cuts) == parts
    pieces = decode_pieces(k, iq, cuts)
    for (r, _), cu in zip(pieces, cuts):
        assert r.status in (0, 2) and r.stream_symbol_offset == cu["sym_off"]
    assert all(r.first_out_symbol == multi.PRE_SYMBOLS for r, _ in pieces[1:])
    st = multi.stitch_ts(pieces, d)
    assert len(st) == len(ref) and (st == ref).all(), (parts, len(st), len(ref))


# ---- (b) the streaming entry, world 1

@pytest.mark.parametrize("k", CELLS, ids=cell_id)
def test_stream_equals_one_chain(po, k):
    iq, ref, _ = single_chain(po, k)
    call, device = call_size(k), k.no % 2 == 1
    t0 = time.perf_counter()
    st = g.RxStream(k.const, k.cr, k.mode, segment_superframes=1, guard=k.guard)
    ts, info, in_flight, trace, _ = run_stream(st, iq, call, device=device)
    print(f"streamed {cell_id(k)}: call {call} samples ({'device' if device else 'host'} pushes), pieces_in_flight <= {in_flight}, {time.perf_counter() - t0:.2f} s")
    assert info.status & ~2 == 0, info.status
    assert len(ts) == len(ref) > 0, (len(ts), len(ref), trace)
    assert (ts == ref).all(), (int(np.flatnonzero(ts != ref)[0]) // 188, trace)
    assert info.finished and info.ts_bytes_pulled == len(ref) and info.ts_bytes_ready == 0
    pieces_decoded_the_body(in_flight, trace)


# ---- (c) sharded, clean streams: status bit 5 has no reason to be raised, there is no way out

def run_sharded(k, iq, world, call, seg_sf=1):
    ranks = [g.RxStream(k.const, k.cr, k.mode, segment_superframes=seg_sf, guard=k.guard, rank=r, world=world) for r in range(world)]
    chunks = []
    for a in range(0, len(iq), call):
        for st in ranks:
            st.push(iq[a:a + call])
        for r, st in enumerate(ranks):
            chunks += [(fp, r, b) for fp, b in st.pull_chunks()]
    for r, st in enumerate(ranks):
        st.finish()
        chunks += [(fp, r, b) for fp, b in st.pull_chunks()]
    infos = [st.info() for st in ranks]
    for st in ranks:
        st.close()
    return chunks, infos


@pytest.mark.parametrize("no,world", [(1, 2), (4, 2), (9, 2), (12, 2), (3, 3), (10, 3)])
def test_sharded_stream_equals_one_chain(po, no, world):
    k = cell(no)
    iq, ref, _ = single_chain(po, k)
    t0 = time.perf_counter()
    chunks, infos = run_sharded(k, iq, world, 40 * k.L + 3)
    print(f"sharded {cell_id(k)}: world {world}, call {40 * k.L + 3} samples, {len(chunks)} chunks, {time.perf_counter() - t0:.2f} s")
    assert all(i.status & ~2 == 0 for i in infos), [i.status for i in infos]
    chunks.sort(key=lambda t: t[0])
    # contiguous from the stream's first packet, no packet twice, every rank contributed
    at = infos[0].first_ts_packet
    assert chunks[0][0] == at
    for fp, r, b in chunks:
        assert fp == at and len(b) % 188 == 0, (fp, at, r)
        at += len(b) // 188
    assert len({r for _, r, _ in chunks}) == world
    ts = np.concatenate([b for _, _, b in chunks])
    assert len(ts) == len(ref) > 0 and (ts == ref).all()


# ---- (d) a lost lock at other guards, world 1

@pytest.mark.parametrize("const,cr,mode,guard,nsf,hole_symbol", [
    (g.QAM16, g.C2_3, g.T2k, g.G1_4, 10, 272 * 5 + 100),
    (g.QPSK, g.C1_2, g.T2k, g.G1_8, 10, 272 * 6 + 40),
    (g.QAM64, g.C5_6, g.T2k, g.G1_16, 10, 272 * 4 + 200),
    (g.QAM64, g.C3_4, g.T8k, g.G1_16, 8, 272 * 4 + 100),
    (g.QAM16, g.C7_8, g.T8k, g.G1_4, 8, 272 * 3 + 150),
    (g.QPSK, g.C3_4, g.T8k, g.G1_8, 8, 272 * 5 - 20),
])
def test_lock_lost_inside_a_piece_is_the_single_chain(po, const, cr, mode, guard, nsf, hole_symbol):
    """30 symbols of silence in the middle of the stream: the pieces are left where the lock is lost, the walk follows the reference through the re-acquisition
    and pieces take over again -- with every offset of that hand-over counted in symbols of another length"""
    c = po.cfg(const, cr, mode, guard)
    L = c.N + c.cp
    iq = streamcases.holed(po, c, nsf, hole_symbol, 9)
    o = po.rx(c, iq, want=("ts",))
    ref = o["ts"]
    assert len(o["lock_periods"]) == 2                                       # the input is the case it claims to be
    _, single = hip_single_chain(const, cr, mode, guard, iq)
    assert len(single) == len(ref) > 0 and (single == ref).all(), "HIP single chain differs from the oracle"
    t0 = time.perf_counter()
    st = g.RxStream(const, cr, mode, segment_superframes=2 if mode == g.T2k else 1, guard=guard)
    ts, info, in_flight, trace, _ = run_stream(st, iq, 64 * L)
    print(f"lost lock {streamcases.name(const, cr, mode, guard)}: call {64 * L} samples, pieces_in_flight <= {in_flight}, {time.perf_counter() - t0:.2f} s")
    assert info.status & 2 and not info.status & 32, info.status
    assert len(ts) == len(ref), (len(ts), len(ref), trace)
    assert (ts == ref).all(), (int(np.flatnonzero(ts != ref)[0]) // 188, trace)


# ---- (e) the options, each at a guard other than 1/32

@pytest.mark.parametrize("no", [1, 9])
def test_auto_configured_stream(po, no):
    """constellation, hierarchy and code rate read from the stream's TPS word: how much of the head that takes (auto_need) is counted in symbols of L samples"""
    k = cell(no)
    iq, ref, _ = single_chain(po, k)
    st = g.RxStream(g.AUTO, g.AUTO, k.mode, segment_superframes=1, guard=k.guard, hierarchy=g.AUTO)
    ts, info, in_flight, trace, _ = run_stream(st, iq, 40 * k.L)
    assert info.auto_configured == 1 and (info.constellation, info.hierarchy, info.code_rate) == (k.const, g.NH, k.cr)
    assert info.status & ~2 == 0 and info.finished
    assert len(ts) == len(ref) and (ts == ref).all(), (len(ts), len(ref), trace)
    pieces_decoded_the_body(in_flight, trace)


def test_soft_decision_stream(po):
    """a clean signal decodes to the same bytes with soft decisions"""
    k = cell(4)
    iq, ref, _ = single_chain(po, k)
    st = g.RxStream(k.const, k.cr, k.mode, segment_superframes=1, guard=k.guard, soft_decision=1)
    ts, info, in_flight, trace, _ = run_stream(st, iq, 64 * k.L)
    assert info.status & ~2 == 0 and info.finished
    assert len(ts) == len(ref) and (ts == ref).all(), (len(ts), len(ref), trace)
    pieces_decoded_the_body(in_flight, trace)


def test_borrowed_device_pushes(po):
    """the samples stay where the caller has them: the release point only moves forward, and it moves"""
    k = cell(11)
    iq, ref, _ = single_chain(po, k)
    st = g.RxStream(k.const, k.cr, k.mode, segment_superframes=1, guard=k.guard, borrow=1)
    ts, info, in_flight, trace, rel = run_stream(st, iq, 64 * k.L, device=True, pull_every=1)
    assert info.status & ~2 == 0 and info.finished
    assert len(ts) == len(ref) and (ts == ref).all(), (len(ts), len(ref), trace)
    assert all(b >= a for a, b in zip(rel, rel[1:])) and 0 < rel[-1] <= len(iq)
    pieces_decoded_the_body(in_flight, trace)


def test_three_chains_pushed_without_a_pull(po):
    """three chains take the pieces in turn; nothing is pulled before the stream has ended: every piece is harvested because its handle is needed again"""
    k = cell(2)
    iq, ref, _ = single_chain(po, k)
    st = g.RxStream(k.const, k.cr, k.mode, segment_superframes=1, guard=k.guard, chains=3)
    ts, info, in_flight, trace, _ = run_stream(st, iq, 33 * k.L + 5, pull_every=1 << 30)
    assert info.status & ~2 == 0 and info.finished
    assert len(ts) == len(ref) and (ts == ref).all(), (len(ts), len(ref), trace)
    assert in_flight >= 2, trace                                              # two pieces decode while the third fills
    pieces_decoded_the_body(in_flight, trace)
