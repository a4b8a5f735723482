"""The float64 references of tests/txref.py against the oracle (CPU only): the GPU transmit tests rest on them.

The baseband helper must give the oracle generator's output (po.tx) from the oracle's own frequency-domain frames, and the shifted transforms
must be the oracle's o_ifft_shift / o_fft_forward_shift, at both transmission modes; the TPS decoder must read back the word o_tps_format
writes, and the BCH remainder must be zero on it.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import txref  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("const,cr,mode,guard", [(1, 0, 0, 0), (2, 4, 1, 3), (0, 2, 1, 1), (2, 1, 0, 2)])
def test_baseband64_is_the_oracle_generator(po, const, cr, mode, guard):
    c = po.cfg(const, cr, mode, guard=guard)
    npk = po.packets_per_superframe(c) // 4 + 5
    scale = 0.0022097087
    iq, freq = po.tx(c, po.make_ts(npk, 2), scale=scale, want_freq=True)
    assert freq.shape[0] > 8
    ref = txref.baseband64(freq, c.cp, scale)
    assert ref.shape == iq.shape
    # the oracle rounds its double IFFT to float once, then scales in float: a few float32 ulps of the peak
    assert np.abs(iq - ref).max() <= 1e-6 * np.abs(ref).max()
    assert txref.rel_rms(iq, ref) < 1e-6
    f32 = txref.baseband32(freq, c.cp, scale)
    r32 = txref.rel_rms(f32, ref)
    assert 0 < r32 < 1e-6                                                 # the calibration figure: a float32 FFT, not zero and not gross


@pytest.mark.parametrize("N", [64, 2048, 8192])
def test_shifted_transforms_are_the_oracles(po, N):
    L = po.lib()
    rng = np.random.RandomState(N)
    x = (rng.randn(3, N) + 1j * rng.randn(3, N)).astype(np.complex64)
    inv, fwd = np.zeros_like(x), np.zeros_like(x)
    for i in range(3):
        L.o_ifft_shift(N, _p(x[i]), _p(inv[i]))
        L.o_fft_forward_shift(N, _p(x[i]), _p(fwd[i]))
    for out, forward in ((inv, False), (fwd, True)):
        ref = txref.fft64(x, forward)
        assert np.abs(out - ref).max() <= 1e-6 * np.abs(ref).max(), (N, forward)
        assert 0 < txref.rel_rms(txref.fft32(x, forward), ref) < 1e-6
    # single bins: the tone of the bin, with the half-spectrum shift
    for b in (0, 1, 5, N // 2 - 1, N // 2, N - 1):
        e = np.zeros(N, np.complex64)
        e[b] = 1
        for forward in (False, True):
            assert np.abs(txref.fft64(e, forward) - txref.single_bin_output(N, b, forward)).max() < 1e-10, (b, forward)


@pytest.mark.parametrize("const,hier,cr,guard,mode,cid_on,cid", [(2, 0, 4, 0, 1, 0, 0), (1, 2, 1, 3, 0, 1, 0x5a), (0, 0, 2, 1, 0, 0, 0)])
def test_tps_decoder_reads_the_oracle_word(po, const, hier, cr, guard, mode, cid_on, cid):
    c = po.cfg(const, cr, mode, guard=guard, hierarchy=hier, include_cell_id=cid_on, cell_id=cid)
    npk = po.packets_per_superframe(c) + 3
    _, freq = po.tx(c, po.make_ts(npk, 4), scale=1.0, want_freq=True)
    car, wk = txref.tps_carriers(po, c)
    wk_all = np.zeros(c.Kmax + 1, np.int8)
    po.lib().o_prbs_wk(C.byref(c), _p(wk_all))
    for f in range(4):
        t = txref.decode_tps(freq[68 * f:68 * (f + 1)], c.zeros_left, car, wk)
        ref = np.zeros(68, np.uint8)
        po.lib().o_tps_format(C.byref(c), f, _p(wk_all), _p(ref))
        assert t[0] == 0 and (t[1:] == ref[1:]).all(), f
        assert txref.bch_remainder(t[1:]) == 0
        assert txref.tps_field(t, 23, 24) == f and txref.tps_field(t, 25, 26) == const and txref.tps_field(t, 30, 32) == cr
    bad = t.copy()
    bad[40] ^= 1
    assert txref.bch_remainder(bad[1:]) != 0
