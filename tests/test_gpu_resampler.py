"""resample_scale_kernel (k_resample.hpp) behind the resampler block and the segment path, at every kind of ratio the library accepts: down- and
up-sampling, the ratios that fill the kernel's input tile (5/13: 753 of 768 samples) and its branch table (93/1: 3069 of 3072 floats) to the edge,
launches of 1, 255, 256, 257 outputs, a stream fed one sample at a time while the history is shorter than a branch, both entries.

Impulses are compared bit for bit (a shifted tile or a transposed branch table moves a tap, which noise under a tolerance can hide).  A Gaussian stream
is compared output by output with the float64 reference of tests/rxref.py under the derived bound rxref.resample_bound, and bit for bit between the
entries and between call schedules: a split must not change a sample.  What every call produces is checked against a rule written from the block's
contract (rxref.resampler_call_count).  tests/test_resampler_ref.py pins the reference to the oracle without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rxref  # noqa: E402

pytestmark = pytest.mark.gpu

RATIOS = [(64, 70), (70, 64), (1, 1), (1, 2), (2, 1), (3, 2), (2, 5), (5, 13), (93, 1), (93, 92)]
REFUSED = [(94, 1), (3, 8), (35, 93), (1, 93)]                  # tests/test_resampler_ref.py::test_support_table
NONPOSITIVE = [(0, 70), (64, 0), (-64, 70), (64, -70), (-64, -70)]
SCALE = 0.37                                                    # not a power of two: the final multiplication rounds
ENTRIES = ("host", "device")
NOUT_CYCLE = (1, 255, 256, 257, 511, 513, 1000)                 # around one and two workgroups of 256 outputs
SLACK = 1024                                                    # output room behind the stream's last sample: more than any entry of NOUT_CYCLE


def _ids(cases):
    return ["/".join(str(v) for v in c) for c in cases]


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0
    return gr_dvbt_amd


@pytest.fixture(scope="module")
def dev():
    """device buffers on one HIP stream: the whole input goes up once, every call reads and writes at its offset, the output comes back after the
    stream has drained"""
    import torch

    class Dev:
        def __init__(self):
            self.s = torch.cuda.Stream()

        def up(self, a):
            with torch.cuda.stream(self.s):
                return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda", non_blocking=False)

        def buf(self, nbytes):
            with torch.cuda.stream(self.s):
                return torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")

        def down(self, t, nbytes):
            self.s.synchronize()
            return t[:nbytes].cpu().numpy()
    return Dev()


def _design(g, interp, decim, scale=SCALE):
    """a block and what dvbt_resampler_get_taps says of it: (block, float32 taps, ri, rd, nt)"""
    b = g.Block("resampler", interp, decim, scale)
    fn = b.L.dvbt_resampler_get_taps
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    ri, rd = C.c_int(), C.c_int()
    n = fn(b.h, None, 0, C.byref(ri), C.byref(rd))
    assert n > 0
    taps = np.zeros(n, np.float32)
    assert fn(b.h, taps.ctypes.data_as(C.c_void_p), n, None, None) == n
    return b, taps, ri.value, rd.value, -(-n // ri.value)


# ---------------------------------------------------------------- call schedules: (nout, nin) of the next call from the stream position
def _ample_in(b, nout):
    return b.forecast(nout) + 8


def _ample_out(ri, rd, nin):
    return nin * ri // rd + ri + 8                              # more than the ceil(nin ri / rd) + 1 outputs that nin inputs can complete


def sched_output_limited(b, ri, rd, nt):
    """(a) nout cycling through NOUT_CYCLE, more input offered than it needs; what is not consumed is offered again"""
    def nxt(k):
        nout = NOUT_CYCLE[k % len(NOUT_CYCLE)]
        return nout, _ample_in(b, nout)
    return nxt


def sched_input_limited(b, ri, rd, nt):
    """(b) 150 calls of one sample from the stream start (the history is shorter than nt - 1 for every nt up to 86 and beyond), then calls around a
    branch length and large ones, then the rest; more output room than the input can fill"""
    nins = [1] * 150 + [2, nt - 2, nt - 1, nt, 35, 1000, 70001]

    def nxt(k):
        nin = nins[k] if k < len(nins) else 1 << 20
        return _ample_out(ri, rd, nin), nin
    return nxt


def sched_mixed(b, ri, rd, nt):
    """(c) a seeded mix of both kinds"""
    rng = np.random.RandomState(1000 * ri + rd)
    nins = (1, 2, nt - 1, nt, 35, 1000, 4097)

    def nxt(k):
        if rng.randint(2):
            nout = NOUT_CYCLE[rng.randint(len(NOUT_CYCLE))]
            return nout, _ample_in(b, nout)
        nin = nins[rng.randint(len(nins))]
        return _ample_out(ri, rd, nin), nin
    return nxt


def sched_one_call(b, ri, rd, nt):
    return lambda k: (1 << 30, 1 << 30)


def run_stream(g, dev, entry, interp, decim, scale, x, sched):
    """x through a fresh block in the calls of `sched`.  Every call must produce what the call rule says and consume 0 .. nin samples, and one that
    is offered input must get on; the stream must end with every sample consumed and ceil(len ri / rd) outputs.  Returns (the output, the calls
    as (nout, nin, produced, consumed))."""
    b, _, ri, rd, nt = _design(g, interp, decim, scale)
    nxt = sched(b, ri, rd, nt)
    total = -(-len(x) * ri // rd)
    cap = total + SLACK
    if entry == "device":
        xin, dout = dev.up(x), dev.buf(cap * 8)
    outs, calls, pos, produced = [], [], 0, 0
    while pos < len(x) or produced < total:
        assert len(calls) < 100000
        nout, nin = nxt(len(calls))
        nout, nin = min(nout, cap - produced), min(nin, len(x) - pos)
        assert nout >= 1 and nin >= 1, "outputs are missing but the input is used up"
        want = rxref.resampler_call_count(ri, rd, produced, pos, nout, nin)
        if entry == "host":
            o = np.zeros(nout, np.complex64)
            r, cons, _ = b.work(nout, nin, x[pos:pos + nin].copy(), o)
            outs.append(o[:max(r, 0)])
        else:
            r, cons, _ = b.work_device(nout, nin, xin.data_ptr() + pos * 8, dout.data_ptr() + produced * 8, (), dev.s.cuda_stream)
        assert r == want, (len(calls), nout, nin, produced, pos, r, want)
        assert 0 <= cons <= nin and (r > 0 or cons > 0), (len(calls), nout, nin, produced, pos, r, cons)
        calls.append((nout, nin, r, cons))
        pos += cons
        produced += r
    assert pos == len(x) and produced == total
    if entry == "device":
        got = dev.down(dout, cap * 8).view(np.complex64)
        assert not got[total:].view(np.uint32).any(), "written behind the stream's last output"
        got = got[:total].copy()
    else:
        got = np.concatenate(outs)
    b.close()
    return got, calls


def _same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


# ---------------------------------------------------------------- impulses
def _impulse_streams(ri, rd, nt):
    """stream positions of the unit samples, dealt to as few streams as keep them 2 nt apart: the stream start, around the first sample with a full
    history (nt - 2, nt - 1, nt), and the first and last input that the second and the third workgroup of a launch from M = 0 stage
    (k_resample.hpp: n_lo = floor(256 g rd / ri) - (nt - 1), n_hi = floor((256 g + 255) rd / ri)).  Returns (streams, the common length)."""
    pos = {0, nt - 2, nt - 1, nt}
    for wg in (1, 2):
        pos |= {max(256 * wg * rd // ri - (nt - 1), 0), (256 * wg + 255) * rd // ri}
    streams = []
    for p in sorted(pos):
        for s in streams:
            if p - s[-1] >= 2 * nt:
                s.append(p)
                break
        else:
            streams.append([p])
    return streams, max(pos) + 2 * nt + 1


@pytest.mark.parametrize("interp,decim,scale", [(i, d, SCALE) for i, d in RATIOS] + [(64, 70, 0.0), (5, 13, 0.0)],
                         ids=_ids([(i, d, SCALE) for i, d in RATIOS] + [(64, 70, 0.0), (5, 13, 0.0)]))
def test_impulses_bit_for_bit(g, dev, interp, decim, scale):
    """one launch over a stream of unit samples: out[M] = float32(branch tap) * float32(scale) exactly, the imaginary part exactly 0.  A sum of
    zeros and one tap is exact in any order, fused or not, so is its one product with the scale.  Scale 0.0 means 1.0."""
    b, taps, ri, rd, nt = _design(g, interp, decim, scale)
    b.close()
    streams, n = _impulse_streams(ri, rd, nt)
    total = -(-n * ri // rd)
    assert total >= 768                                        # three workgroups
    M = np.arange(total, dtype=np.int64)
    n_of, b_of = M * rd // ri, M * rd % ri
    padded = np.concatenate([taps, np.zeros(ri * nt - len(taps), np.float32)])
    for ps in streams:
        x = np.zeros(n, np.complex64)
        x[ps] = 1.0
        want = np.zeros(total, np.float32)
        for p in ps:
            k = n_of - p
            hit = (k >= 0) & (k < nt)
            want[hit] = padded[b_of[hit] + k[hit] * ri]                  # branch[b][k] = taps[b + k ri]
        want = want * np.float32(scale if scale else 1.0)
        assert want.dtype == np.float32 and np.count_nonzero(want) >= len(ps) * (nt - 1) * ri // rd
        for entry in ENTRIES:
            got, calls = run_stream(g, dev, entry, interp, decim, scale, x, sched_one_call)
            assert len(calls) == 1
            bad = np.flatnonzero((got.real != want) | (got.imag != 0))
            assert not len(bad), (entry, ps, bad[:8], got[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------- Gaussian stream
_STREAM = {}


def _stream(nt):
    """the input of the Gaussian tests: as long as the input-limited schedule needs, and a ragged rest"""
    n = 150 + 2 + (nt - 2) + (nt - 1) + nt + 35 + 1000 + 70001 + 1237
    if n not in _STREAM:
        rng = np.random.RandomState(3)
        _STREAM[n] = (rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)
    return _STREAM[n]


@pytest.mark.parametrize("interp,decim,scale", [(i, d, SCALE) for i, d in RATIOS] + [(3, 2, 0.0)], ids=_ids([(i, d, SCALE) for i, d in RATIOS] + [(3, 2, 0.0)]))
def test_gaussian_stream(po, g, dev, interp, decim, scale):
    """three call schedules through both entries: the call rule at every call, the six streams bitwise equal, and each output within
    rxref.resample_bound of the float64 reference over the block's own float32 taps (test_taps_and_forecast bounds those against the float64
    design).  Prints the worst error / bound of the kernel next to that of the oracle's sequential float32 sums on the same stream."""
    b, taps, ri, rd, nt = _design(g, interp, decim, scale)
    b.close()
    x = _stream(nt)
    runs = {}
    for name, sched in (("output-limited", sched_output_limited), ("input-limited", sched_input_limited), ("mixed", sched_mixed)):
        for entry in ENTRIES:
            runs[name, entry], calls = run_stream(g, dev, entry, interp, decim, scale, x, sched)
            c = np.array(calls)
            if name == "output-limited":                       # the schedule is what it claims: every nout of the cycle was filled to the last sample
                assert {int(v) for v in c[c[:, 0] == c[:, 2], 0]} >= set(NOUT_CYCLE)
            if name == "input-limited":                        # one sample at a time from the stream start, each one consumed
                assert (c[:150, 1] == 1).all() and (c[:150, 3] == 1).all() and c[:150, 2].sum() == -(-150 * ri // rd)
                assert {int(v) for v in c[c[:, 1] == c[:, 3], 1]} >= {2, nt - 2, nt - 1, nt, 35, 1000, 70001}
    first = runs["output-limited", "host"]
    for key, got in runs.items():
        assert _same_bits(got, first), (key, np.flatnonzero(got.view(np.uint64) != first.view(np.uint64))[:8])
    s = float(np.float32(scale)) if scale else 1.0
    ref, a_re, a_im = rxref.resample64(x, taps, ri, rd, s)
    assert len(ref) == len(first)
    q = []
    for got in (first, po.resample(x, interp, decim, s)):
        q_re = np.abs(got.real.astype(np.float64) - ref.real) / rxref.resample_bound(a_re, nt)
        q_im = np.abs(got.imag.astype(np.float64) - ref.imag) / rxref.resample_bound(a_im, nt)
        q.append((q_re, q_im))
    print(f"\n[resampler {interp}/{decim} scale {scale}] {len(x)} -> {len(ref)} samples, nt {nt}: worst error / bound "
          f"{max(q[0][0].max(), q[0][1].max()):.3f} (oracle {max(q[1][0].max(), q[1][1].max()):.3f})")
    assert (q[0][0] <= 1.0).all() and (q[0][1] <= 1.0).all()


# ---------------------------------------------------------------- taps, forecast, refusals
@pytest.mark.parametrize("interp,decim", RATIOS, ids=_ids(RATIOS))
def test_taps_and_forecast(g, interp, decim):
    """the float32 design rounds three times (window, windowed sinc, normalised tap): 4 * 2^-24 of the largest tap, per tap"""
    b, taps, ri, rd, nt = _design(g, interp, decim)
    t64, ri64, rd64, nt64 = rxref.resampler_design64(interp, decim)
    assert (ri, rd, nt, len(taps)) == (ri64, rd64, nt64, len(t64))
    assert (np.abs(taps.astype(np.float64) - t64) <= 4 * 2.0 ** -24 * np.abs(t64).max()).all()
    for n in (1, 255, 3200):
        assert b.forecast(n) == max(1, n * rd // ri + nt - 1)
    b.close()


def _short_run(g, dev, interp, decim):
    rng = np.random.RandomState(9)
    x = (rng.randn(3000) + 1j * rng.randn(3000)).astype(np.complex64)
    got, _ = run_stream(g, dev, "host", interp, decim, SCALE, x, sched_one_call)
    b, taps, ri, rd, nt = _design(g, interp, decim)
    b.close()
    ref, a_re, a_im = rxref.resample64(x, taps, ri, rd, float(np.float32(SCALE)))
    assert (np.abs(got.real - ref.real) <= rxref.resample_bound(a_re, nt)).all() and (np.abs(got.imag - ref.imag) <= rxref.resample_bound(a_im, nt)).all()


def test_refusals(g, dev):
    """a ratio whose design does not fit the kernel's tile or branch table, or that is not positive, fails at create with the invalid-argument
    error, as a block and in front of the chain; a block created afterwards works; the streaming receiver takes no resampler"""
    from gr_dvbt_amd import binding
    for i, d in REFUSED:
        _, ri, rd, nt = rxref.resampler_design64(i, d)
        assert not rxref.resampler_supported(ri, rd, nt)
    for i, d in REFUSED + NONPOSITIVE:
        with pytest.raises(g.DvbtError, match="error -1:"):
            g.Block("resampler", i, d, SCALE)
        with pytest.raises(g.DvbtError, match="error -1:"):
            g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=1 << 20, resample=(i, d), front_scale=SCALE)
    _short_run(g, dev, 64, 70)
    _short_run(g, dev, 5, 13)
    L = g.lib()
    for i, d in ((64, 70), (0, 70), (64, 0)):
        rx = g.RxParams(g.QAM16, g.NH, g.C1_2, g.G1_32, g.T2k, 0, 0, 30.0, 768, 0, 1, 0, 0, 0, i, d, 0.0, 0)
        p, h = binding.StreamParams(rx, 0, 0, 0, 0, 0, 0), C.c_void_p()
        L.dvbt_rx_stream_create.restype = C.c_int
        L.dvbt_rx_stream_create.argtypes = [C.POINTER(binding.StreamParams), C.POINTER(C.c_void_p)]
        assert L.dvbt_rx_stream_create(C.byref(p), C.byref(h)) == -1 and not h.value


# ---------------------------------------------------------------- segment path
@pytest.mark.parametrize("const,cr,mode,nsf,up,down,scale", [
    (2, 4, 1, 2, (70, 64), (64, 70), 0.00055242272),           # 8k QAM64 7/8 from the 10 Msps file format
    (1, 0, 0, 3, (2, 1), (1, 2), 0.0022097087),                # 2k QAM16 1/2 from a file at twice the rate
], ids=["8k-qam64-7_8-64_70", "2k-qam16-1_2-1_2"])
def test_chain_from_file_rate(po, g, const, cr, mode, nsf, up, down, scale):
    """file-rate samples in, TS out (prepare_chain: one launch over the whole segment, then the chain): TS, cp_start and the RS counts identical
    to the oracle chain fed with the oracle-resampled stream.  Clean loopbacks: every decision has margin over the resamplers' float differences."""
    c = po.cfg(const, cr, mode)
    ts = po.make_ts(nsf * po.packets_per_superframe(c), 77)
    iq = po.tx(c, ts, scale=1.0 / (10 * np.sqrt(float(c.N))), lead_in=1000, tail=3 * c.N)
    file_rate = po.resample(iq, up[0], up[1], 1.0)
    o = po.rx(c, po.resample(file_rate, down[0], down[1], scale), want=("ts", "rs"))
    assert o["ts"].size > 100000
    rx = g.Rx(const, cr, mode, max_samples=len(file_rate), resample=down, front_scale=scale, taps=True)
    rep = rx.run(file_rate)
    assert rep.status == 0 or rep.status == 2
    got = rx.tap(g.TAP_TS)
    assert got.size == o["ts"].size and (got == o["ts"]).all()
    # the lead-in's resampled edge can cost the reference its first lock (2/1 then 1/2: periods of 1, 2 and 812 symbols): every period where and as
    # long as the oracle's; the report's n_symbols and the CP_START tap describe the last one (include/dvbt_hip.h)
    L = c.N + c.cp
    assert rep.total_symbols == o["n_acquired"]
    assert [(off + fc * L, n) for (off, fc, cp0, n, fo) in rx.lock_periods() if n > 0] == o["lock_periods"]
    assert rep.n_symbols == o["lock_periods"][-1][1] and (rx.tap(g.TAP_CP_START) == o["cp_start"][o["n_acquired"] - rep.n_symbols:]).all()
    assert rep.rs_fail_words == o["rs_fail"] and rep.rs_corrected_symbols == o["rs_corr"]
    assert (rx.tap(g.TAP_RS) == o["rs"]).all()
    rx.close()
