"""The fused modulator (dvbt_tx_*, gr_dvbt_amd.Tx) over its whole configuration space, against the oracle's generator and a float64 reference.

- every (constellation, code rate, mode), the guard interval, the cell id and the dispersal phase rotated through them;
- every hierarchy value with every constellation (QPSK included: the oracle and the reference give hierarchical QPSK the same meaning, alpha added to
  the level with the QPSK norm, so it is tested like the rest);
- one stream split over calls of 0, 1, 127, 128, 129 packets and one across a superframe boundary, host and device entries alternating;
- first_packet and first_packet + 8 * 2^40 (the same dispersal phase).

The carriers (the IFFT input) must be bit-exact with the oracle's frames.  The baseband is compared with numpy's complex128 IFFT of those frames
(txref.baseband64): the maximum error within 1e-5 of the peak, and the relative RMS error within RMS_K times that of a complex64 IFFT of the same
frames on the CPU (txref.baseband32), so that the bound follows the accuracy of an ordinary float32 FFT instead of a constant.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import txref  # noqa: E402

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

RMS_K = 6.0                 # GPU relative RMS error <= RMS_K x that of a float32 FFT (measured on MI355X: 1.9 - 2.2 at N = 2048, 3.4 - 4.0 at 8192)
SCALE = 0.0022097087


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    return gr_dvbt_amd


def _check_baseband(iq, car, cp, scale, what):
    """iq (GPU) against the float64 baseband of the exact carriers car: max error and the self-calibrating RMS bound"""
    ref = txref.baseband64(car, cp, scale)
    assert iq.shape == ref.shape and len(ref) > 0
    assert np.abs(iq - ref).max() <= 1e-5 * np.abs(ref).max(), what
    r_gpu = txref.rel_rms(iq, ref)
    r_f32 = txref.rel_rms(txref.baseband32(car, cp, scale), ref)
    print(f"\nrms {what} N={car.shape[1]} gpu={r_gpu:.3e} f32={r_f32:.3e} ratio={r_gpu / r_f32:.2f}")
    assert r_gpu <= RMS_K * r_f32, (what, r_gpu, r_f32)


def _run_case(po, g, const, cr, mode, guard, hier, cid_on, cid, fp, seed):
    c = po.cfg(const, cr, mode, guard=guard, hierarchy=hier, include_cell_id=cid_on, cell_id=cid)
    npk = 2 * po.packets_per_superframe(c) + 37                      # two superframes and an odd tail
    ts = po.make_ts(npk, seed)
    iq_ref, freq_ref = po.tx(c, ts, scale=SCALE, want_freq=True, packet0=fp)
    assert len(freq_ref) >= 2 * 4 * 68
    tx = g.Tx(const, cr, mode, guard=guard, hierarchy=hier, include_cell_id=cid_on, cell_id=cid, scale=SCALE, max_packets=npk, first_packet=fp,
              keep_carriers=True)
    assert tx.samples_for(npk) == len(iq_ref)
    iq = tx.run(ts)
    car = tx.carriers()
    tx.close()
    assert car.shape == freq_ref.shape
    assert car.view(np.uint64).tobytes() == freq_ref.view(np.uint64).tobytes()
    _check_baseband(iq, freq_ref, c.cp, SCALE, f"tx c{const} r{cr} m{mode} g{guard} h{hier}")


# every (constellation, code rate, mode): guard = (const + cr + mode) mod 4 meets every mode and every constellation with every guard
SWEEP = [(const, cr, mode) for const in range(3) for cr in range(5) for mode in range(2)]


@pytest.mark.parametrize("const,cr,mode", SWEEP)
def test_every_configuration(po, g, const, cr, mode):
    guard = (const + cr + mode) % 4
    cid_on = (cr + mode) % 2
    rng = np.random.RandomState(100 * const + 10 * cr + mode)
    cid = int(rng.randint(0, 256))
    fp = int(rng.randint(0, 16))
    _run_case(po, g, const, cr, mode, guard, 0, cid_on, cid, fp, seed=20 + 10 * const + 2 * cr + mode)


HIER = [(const, hier, mode) for const in (1, 2) for hier in (1, 2, 3) for mode in (0, 1)] + [(0, hier, 0) for hier in (1, 2, 3)]


@pytest.mark.parametrize("const,hier,mode", HIER)
def test_hierarchical_modes(po, g, const, hier, mode):
    cr = (const + hier + mode) % 5
    guard = (hier + mode) % 4
    fp = (5 * hier + const) % 16
    _run_case(po, g, const, cr, mode, guard, hier, mode, 0x40 + hier, fp, seed=60 + 7 * const + hier + mode)


# ---------------------------------------------------------------- splits
SPLIT = [(0, 0, 0), (1, 1, 0), (2, 2, 0), (0, 3, 1), (1, 4, 1), (2, 1, 1)]    # (const, cr, mode): one per (mode, constellation)


@pytest.mark.skipif(torch is None, reason="needs torch")
@pytest.mark.parametrize("const,cr,mode", SPLIT)
def test_split_over_calls_equals_one_call(po, g, const, cr, mode):
    c = po.cfg(const, cr, mode)
    pps = po.packets_per_superframe(c)
    # after 385 packets, a call of one superframe's packets crosses the boundary at pps
    sizes = [129, 0, 1, 127, 128, pps, 77, 124]
    npk = sum(sizes)
    ts = po.make_ts(npk, 40 + const + mode)
    one = g.Tx(const, cr, mode, scale=SCALE, max_packets=npk, first_packet=3, keep_carriers=True)
    iq_one = one.run(ts)
    car_one = one.carriers()
    one.close()
    tx = g.Tx(const, cr, mode, scale=SCALE, max_packets=max(sizes), first_packet=3, keep_carriers=True)
    dts = torch.from_numpy(ts).cuda()
    outs, cars, p = [], [], 0
    for i, n in enumerate(sizes):
        want = tx.samples_for(n)
        if i % 2 == 0:
            o = tx.run(ts[p * 188:(p + n) * 188])
        else:
            dout = torch.zeros(2 * max(want, 1), dtype=torch.float32, device="cuda")
            got = tx.run_device(dts.data_ptr() + p * 188, n, dout.data_ptr(), want)
            assert got == want
            o = dout.cpu().numpy().view(np.complex64)[:got]
        assert len(o) == want
        cr_ = tx.carriers()
        assert cr_.shape[0] * (c.N + c.cp) == want
        outs.append(o)
        cars.append(cr_)
        p += n
    tx.close()
    assert np.concatenate(outs).tobytes() == iq_one.tobytes()
    assert np.concatenate(cars).tobytes() == car_one.tobytes()
    # and the one call is the oracle's stream
    iq_ref, freq_ref = po.tx(c, ts, scale=SCALE, want_freq=True, packet0=3)
    assert car_one.tobytes() == freq_ref.tobytes()


def test_first_packet_sets_only_the_dispersal_phase(po, g):
    c = po.cfg(0, 0, 0, guard=1)
    npk = po.packets_per_superframe(c) + 300                          # calls of 200 and 352 packets: 2 and 3 workgroups of tx_outer_kernel
    ts = po.make_ts(npk, 9)
    f = 11
    outs = []
    for fp in (f, f + 8 * 2 ** 40):
        tx = g.Tx(0, 0, 0, guard=1, scale=SCALE, max_packets=npk, first_packet=fp, keep_carriers=True)
        outs.append((tx.run(ts[:200 * 188]), tx.run(ts[200 * 188:]), tx.carriers()))
        tx.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    _, freq_ref = po.tx(c, ts, scale=SCALE, want_freq=True, packet0=f)
    assert outs[0][2].tobytes() == freq_ref[-len(outs[0][2]):].tobytes()
    # a different phase is a different stream
    tx = g.Tx(0, 0, 0, guard=1, scale=SCALE, max_packets=npk, first_packet=f + 1, keep_carriers=True)
    tx.run(ts)
    assert tx.carriers().tobytes() != freq_ref.tobytes()
    tx.close()
