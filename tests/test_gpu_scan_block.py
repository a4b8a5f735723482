"""GPU: the signal scanner (dvbt_scan_*) against tests/scanref.py.  The folded sums are compared bit for bit -- the model adds the same float32 terms in the
same order -- at stream lengths on both sides of the first symbol, of the verdict's minimum and of a group's close; what a stream looks like cut into
calls, through the host or the device entry, on two streams, across a read or after a reset is compared bit for bit as well.  End to end, the detected mode
and guard build the receiver that the true parameters build."""
import ctypes as C

import numpy as np
import pytest

import scanref

pytestmark = pytest.mark.gpu

LONGEST = 17 * 10240 + 8192 + 5
LENGTHS = (0, 1, scanref.MIN_SAMPLES - 1, 16 * 10240 + 8192 - 1, 16 * 10240 + 8192 + 1, LONGEST)
CALLS = (1, 2111, 2112, 2113, 10239, 18433)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    return gr_dvbt_amd


@pytest.fixture(scope="module")
def stream():
    """seeded Gaussian samples with a 60 dB level step in the middle"""
    rng = np.random.RandomState(20)
    x = (rng.randn(LONGEST) + 1j * rng.randn(LONGEST)) * np.where(np.arange(LONGEST) < LONGEST // 2, 1e-3, 1.0)
    return x.astype(np.complex64)


@pytest.fixture(scope="module")
def model(stream):
    """{length: [(J, A, E)] * 8} of the float32 model, computed once"""
    return {n: [scanref.fold32(stream[:n], h) for h in range(8)] for n in LENGTHS}


def _bits(s):
    """every hypothesis' sums and the reading's figures, as bytes"""
    r = s.read()
    acc = tuple(v.tobytes() for h in range(8) for v in s.accumulators(h))
    return acc, (r.detected, r.mode, r.guard, r.samples_pushed, r.nonfinite, tuple(r.symbols), tuple(r.symbol_start),
                 np.array(r.rho).tobytes(), np.array(r.cfo).tobytes())


def _cuts(n):
    out, a, i = [], 0, 0
    while a < n:
        b = min(n, a + CALLS[i % len(CALLS)])
        out.append((a, b))
        a, i = b, i + 1
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_accumulators_are_the_models_bit_for_bit(g, stream, model, n):
    s = g.Scanner()
    s.push(stream[:n])
    r = s.read()
    assert r.samples_pushed == n and r.nonfinite == 0
    assert r.symbols == [scanref.symbols(n, h) for h in range(8)] == [m[0] for m in model[n]]
    for h in range(8):
        A, E = s.accumulators(h)
        J, wA, wE = model[n][h]
        assert A.tobytes() == wA.tobytes() and E.tobytes() == wE.tobytes(), (n, h, J)
    want = scanref.evaluate([m[0] for m in model[n]], [m[1] for m in model[n]], [m[2] for m in model[n]], n)
    assert (int(r.detected), r.mode, r.guard) == (want["detected"], want["mode"], want["guard"]) == (0, -1, -1)
    assert r.symbol_start == want["symbol_start"]
    assert np.allclose(r.rho, want["rho"], rtol=1e-12, atol=0) and np.allclose(r.cfo, want["cfo"], rtol=1e-12, atol=0)
    s.close()
    if n == LONGEST:
        assert r.symbols[0] == 5 * 16 + 5 and r.symbols[7] == 16 + 1            # five closed groups and an open one at 2k 1/32; one and an open one at 8k 1/4


@pytest.fixture(scope="module")
def whole(g, stream):
    s = g.Scanner()
    s.push(stream)
    bits = _bits(s)
    s.close()
    return bits


def test_split_host_calls_equal_one_call_bit_for_bit(g, stream, whole):
    s = g.Scanner()
    for a, b in _cuts(LONGEST):
        s.push(stream[a:b])
    assert _bits(s) == whole
    s.close()


def test_split_device_calls_on_two_streams_equal_one_call_bit_for_bit(g, stream, whole):
    import torch
    d = torch.from_numpy(stream.view(np.float32).copy()).to(torch.device("cuda:0"))
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    torch.cuda.synchronize()
    s = g.Scanner()
    for i, (a, b) in enumerate(_cuts(LONGEST)):
        s.push_device(d.data_ptr() + 8 * a, b - a, stream=streams[i & 1].cuda_stream)
    assert _bits(s) == whole                      # read synchronises with whatever stream pushed last
    s.close()
    torch.cuda.synchronize()


def test_read_does_not_disturb_and_reset_starts_again(g, stream, whole):
    s = g.Scanner()
    s.push(stream[:100000])
    mid = _bits(s)
    assert mid == _bits(s)
    s.push(stream[100000:])
    assert _bits(s) == whole
    s.reset()
    r = s.read()
    assert r.samples_pushed == 0 and r.symbols == [0] * 8 and not any(s.accumulators(3)[1])
    for a, b in _cuts(LONGEST)[:9]:
        s.push(stream[a:b])
    s.push(stream[_cuts(LONGEST)[8][1]:])
    assert _bits(s) == whole                      # a reset handle is a fresh one
    s.close()


def test_refused_calls_leave_the_stream_where_it_was(g, stream, whole):
    s = g.Scanner()
    s.push(stream[:50001])
    iq = np.zeros(9, np.complex64)
    with pytest.raises(g.DvbtError):              # a buffer that is not 8-byte aligned
        g.binding._chk(s.L.dvbt_scan_push(s.h, C.c_void_p(iq.ctypes.data + 4), 4))
    with pytest.raises(g.DvbtError):
        g.binding._chk(s.L.dvbt_scan_push(s.h, None, 4))
    with pytest.raises(g.DvbtError):
        s.accumulators(8)
    with pytest.raises(g.DvbtError):
        g.binding._chk(s.L.dvbt_scan_accumulators(s.h, 7, np.zeros(2).ctypes.data_as(C.POINTER(C.c_double)), np.zeros(2).ctypes.data_as(C.POINTER(C.c_double)), 10239))
    s.push(stream[:0])
    s.push(stream[50001:])
    assert _bits(s) == whole
    s.close()


def test_inf_and_nan_are_counted_and_give_no_verdict(g, po):
    c = po.cfg(po.QAM16, po.C2_3, po.T2k, po.G1_8)
    iq = po.tx(c, po.make_ts(po.packets_per_superframe(c), 5), scale=1.0)[:scanref.MIN_SAMPLES + 5000].copy()
    clean = g.Scanner.detect(iq)
    assert clean.detected and (clean.mode, clean.guard) == (po.T2k, po.G1_8) and clean.nonfinite == 0
    iq[70000] = np.inf
    iq[70001] = complex(0.0, np.nan)
    iq[len(iq) - 1] = complex(-np.inf, np.nan)   # one sample, counted once; in no complete symbol of most hypotheses
    r = g.Scanner.detect(iq)
    assert r.nonfinite == 3 and not r.detected and (r.mode, r.guard) == (-1, -1)
    want = scanref.scan(iq)
    assert want["nonfinite"] == 3 and want["detected"] == 0
    assert [np.isnan(v) for v in r.rho] == [np.isnan(v) for v in want["rho"]]
    with pytest.raises(g.DvbtError):
        r.rx_stream()


@pytest.mark.parametrize("mode,guard", ((0, 2), (1, 0)))
def test_detected_parameters_build_the_receiver_of_the_true_ones(g, po, mode, guard):
    """QAM16 2/3 with a carrier offset of 0.3 at 20 dB through Scanner.detect and ScanReading.rx_stream(): the TS is that of an RxStream created with the
    true parameters, byte for byte.  Two superframes go in, which is what it takes for one superframe's TS to come out."""
    c = po.cfg(po.QAM16, po.C2_3, mode, guard)
    iq = po.tx(c, po.make_ts(2 * po.packets_per_superframe(c), 5), lead_in=500, tail=3 * c.N)
    iq = po.channel(iq, c.N, cfo=0.3, snr_db=20.0, seed=5)
    r = g.Scanner.detect(iq)
    h = 4 * mode + guard
    assert r.detected and (r.mode, r.guard) == (mode, guard), r
    assert abs(r.cfo[h] - 0.3) < 0.01 and r.symbol_start[h] == 500 % (c.N + c.cp)
    out = []
    for st in (r.rx_stream(segment_superframes=1), g.RxStream(g.QAM16, g.C2_3, mode, segment_superframes=1, guard=guard)):
        st.push(iq)
        st.finish()
        out.append(st.pull())
        info = st.info()
        st.close()
        assert (info.constellation, info.hierarchy, info.code_rate) == (g.QAM16, g.NH, g.C2_3)
    assert len(out[0]) == len(out[1]) > 0 and (out[0] == out[1]).all()
