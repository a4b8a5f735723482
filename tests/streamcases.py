"""The cases the cut, streamed and sharded receivers are tested at away from guard 1/32 (tests/test_cut_stitch.py on the CPU, tests/test_gpu_stream_matrix.py
on the GPU): every guard interval other than 1/32 in both modes, all five code rates, 12 of the 15 (constellation, rate) pairs.  What moves with them in
csrc/dvbt_stream.inc and gr_dvbt_amd/multi.py: L = N + cp (every sample offset of the plan), the post-roll (8 symbols at 64-QAM 7/8, 90 at QPSK 1/2 -- the
only one longer than the pre-roll of 76), the decoded bits per symbol and packets per superframe (the descrambler's call grid, the chunk labels).

A plain module: the table, the streams with a dropout, and a per-process cache of (samples, oracle TS) so that the tests of one cell generate and
oracle-decode a stream once."""
import collections

import numpy as np

import gr_dvbt_amd as g

Cell = collections.namedtuple("Cell", "no const cr mode guard L post")

#        #   const    rate     mode   guard    L     post-roll (symbols)
CELLS = [Cell(*t) for t in (
    (1, g.QPSK, g.C1_2, g.T2k, g.G1_4, 2560, 90),      # the post-roll is longer than the pre-roll
    (2, g.QPSK, g.C3_4, g.T2k, g.G1_16, 2176, 61),     # 283.5 decoded bytes per symbol
    (3, g.QAM16, g.C2_3, g.T2k, g.G1_8, 2304, 36),
    (4, g.QAM64, g.C5_6, g.T2k, g.G1_4, 2560, 21),
    (5, g.QAM16, g.C7_8, g.T2k, g.G1_16, 2176, 28),
    (6, g.QAM64, g.C1_2, g.T2k, g.G1_8, 2304, 32),
    (7, g.QPSK, g.C2_3, g.T8k, g.G1_16, 8704, 20),
    (8, g.QAM16, g.C5_6, g.T8k, g.G1_8, 9216, 10),
    (9, g.QAM64, g.C7_8, g.T8k, g.G1_4, 10240, 8),     # d_fi_start = 2: the first superframe start is symbol 204
    (10, g.QPSK, g.C7_8, g.T8k, g.G1_8, 9216, 16),
    (11, g.QAM16, g.C1_2, g.T8k, g.G1_4, 10240, 14),
    (12, g.QAM64, g.C3_4, g.T8k, g.G1_16, 8704, 8),    # d_fi_start = 2
)]
SEED = 11

_NAMES = {"const": {g.QPSK: "qpsk", g.QAM16: "qam16", g.QAM64: "qam64"}, "cr": {g.C1_2: "1/2", g.C2_3: "2/3", g.C3_4: "3/4", g.C5_6: "5/6", g.C7_8: "7/8"},
          "mode": {g.T2k: "2k", g.T8k: "8k"}, "guard": {g.G1_32: "g1/32", g.G1_16: "g1/16", g.G1_8: "g1/8", g.G1_4: "g1/4"}}


def name(const, cr, mode, guard):
    return " ".join(_NAMES[k][v] for k, v in (("mode", mode), ("const", const), ("cr", cr), ("guard", guard)))


def cell_id(cell):
    return f"cell {cell.no}: " + name(cell.const, cell.cr, cell.mode, cell.guard)


def cell(no):
    return CELLS[no - 1]


def first_superframe_symbol(const, mode):
    """where the reference's demodulator declares the first superframe start of a stream that begins with a superframe (d_fi_start = 2 in 8k 64-QAM:
    one frame early)"""
    return 204 if (const == g.QAM64 and mode == g.T8k) else 272


def cut_size(cell):
    """(superframes, pieces) of the cut tests"""
    return (6, 3) if cell.mode == g.T2k else (4, 2)


def stream_size(cell):
    """superframes of the streamed and sharded tests: pieces of one superframe each"""
    return 8 if cell.mode == g.T2k else 7


def holed(po, c, nsf, hole_symbol, seed):
    """the synthetic stream with 30 symbols of silence from `hole_symbol` on: the reference's tracker loses its lock there"""
    iq = po.stream_slice(c, nsf, seed).copy()
    L = c.N + c.cp
    hole = po.STREAM_LEAD_IN + hole_symbol * L
    iq[hole:hole + 30 * L] = 0
    return iq


_streams = {}


def stream(po, cell, nsf=None):
    """(samples, oracle TS) of the cell's stream of `nsf` superframes (stream_size(cell) unless given), generated and decoded by the oracle once per process;
    both arrays are read-only"""
    nsf = stream_size(cell) if nsf is None else nsf
    key = (cell.no, nsf)
    if key not in _streams:
        c = po.cfg(cell.const, cell.cr, cell.mode, cell.guard)
        assert c.N + c.cp == cell.L
        iq = po.stream_slice(c, nsf, SEED)
        o = po.rx(c, iq, want=("ts",))
        assert len(o["lock_periods"]) == 1, "a clean stream: one lock period"
        ts = o["ts"].copy()
        iq.setflags(write=False)
        ts.setflags(write=False)
        _streams[key] = (iq, ts)
    return _streams[key]
