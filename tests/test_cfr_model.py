"""The crest-factor reduction block's numpy model (tests/cfrref.py) alone, on the CPU: what the definition in include/dvbt_hip.h promises, checked on
64 synthetic 2k QAM64 symbols with boosted pilots, threshold 7 dB over the measured mean, 2x oversampling, 4 iterations."""
import numpy as np
import pytest

import cfrref as cr

NSYM, SEED, PAPR_DB = 64, 7, 7.0


@pytest.fixture(scope="module")
def case():
    md = cr.Mode(0, 0)
    iq = cr.synthetic_symbols(md, NSYM, SEED)
    power = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    A = cr.threshold_for(PAPR_DB, power)
    out, ctr = cr.run(md, iq, A, iterations=4, os=2)
    return md, iq, power, A, out, ctr


def _spectra(md, iq):
    return np.fft.fft(np.asarray(iq, np.complex128).reshape(-1, md.symbol)[:, md.G:], axis=1)


def test_every_symbol_is_clipped_and_the_prefix_is_cyclic(case):
    md, iq, power, A, out, ctr = case
    assert ctr["symbols"] == ctr["symbols_clipped"] == NSYM and ctr["symbols_nonfinite"] == 0 and ctr["samples_over"] > NSYM
    rows = out.reshape(-1, md.symbol)
    assert (rows[:, :md.G] == rows[:, md.N:]).all()
    assert ctr["peak_power_in"] > A * A


def test_power_in_unoccupied_bins_is_unchanged(case):
    md, iq, power, A, out, ctr = case
    X0, X = _spectra(md, iq), _spectra(md, out)
    inband = (np.abs(X0[:, md.occupied]) ** 2).sum()
    before, after = (np.abs(X0[:, ~md.occupied]) ** 2).sum(), (np.abs(X[:, ~md.occupied]) ** 2).sum()
    print(f"\nout of band / in band: before {before / inband:.3e}, after {after / inband:.3e}")
    assert abs(after - before) <= 1e-12 * inband
    assert (np.abs(X - X0)[:, ~md.occupied] ** 2).sum() <= 1e-12 * inband


@pytest.mark.parametrize("keep", [0, cr.KEEP_PILOTS, cr.KEEP_TPS, cr.KEEP_PILOTS | cr.KEEP_TPS])
def test_kept_carriers_are_unchanged(case, keep):
    md, iq, power, A, _, _ = case
    iq = iq[:8 * md.symbol]
    out, _ = cr.run(md, iq, A, iterations=4, os=2, keep=keep, first_symbol=3)
    X0, X = _spectra(md, iq), _spectra(md, out)
    scale = np.abs(X0).max()
    for l in range(8):
        kept = md.bins(md.kept(3 + l, keep))
        moved = np.abs(X[l] - X0[l]) > 1e-12 * scale
        assert not moved[kept].any()
        free = md.free(3 + l, keep)
        assert moved[free].mean() > 0.9, "the error passes everywhere else in the band"


def test_oversampling_1_is_the_plain_clip_and_filter_loop(case):
    md, iq, power, A, _, _ = case
    iq = iq[:8 * md.symbol]
    out, _ = cr.run(md, iq, A, iterations=3, os=1, keep=cr.KEEP_PILOTS)
    zl = (md.N - md.K + 1) // 2
    for l in range(8):
        # written from the definition, in the shifted order a modulator uses: carrier c at column zl + c
        u = iq[l * md.symbol + md.G:(l + 1) * md.symbol].astype(np.complex128)
        S0 = np.fft.fftshift(np.fft.fft(u))
        mask = np.zeros(md.N, bool)
        mask[zl:zl + md.K] = True
        for c in list(md.cpilot) + list(range(3 * (l % 4), md.K, 12)):
            mask[zl + c] = False
        S = S0.copy()
        for _ in range(3):
            x = np.fft.ifft(np.fft.ifftshift(S))
            big = np.abs(x) > A
            x[big] *= A / np.abs(x[big])
            S = S0 + mask * (np.fft.fftshift(np.fft.fft(x)) - S0)
        want = np.fft.ifft(np.fft.ifftshift(S))
        got = out[l * md.symbol + md.G:(l + 1) * md.symbol]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("os", [2, 4])
def test_the_phase_sum_is_the_oversampled_transform_on_the_occupied_bins(case, os):
    md, iq, power, A, _, _ = case
    X = _spectra(md, iq[:md.symbol])[0]
    x = cr.phases(md, X, os)
    # the phases interleaved are the signal at os times the rate: the inverse os N-point transform of X on its signed indices
    Z = np.zeros(os * md.N, np.complex128)
    Z[md.kappa % (os * md.N)] = X
    z = np.fft.ifft(Z) * os
    assert np.abs(x.T.reshape(-1) - z).max() <= 1e-12 * np.abs(z).max()
    c = cr.clip(x, A)
    assert (np.abs(c) <= A * (1 + 1e-12)).all() and (np.abs(x) > A).any()
    C = cr.back(md, c, os)
    big = np.fft.fft(c.T.reshape(-1)) / os
    want = big[md.kappa % (os * md.N)]
    assert np.abs(C - want)[md.occupied].max() <= 1e-12 * np.abs(want).max()


def test_interpolated_peak_after_the_block(case):
    """The highest 8x-interpolated symbol peak after the block.  The float64 prototype gave threshold + 1.05 dB on its own symbols and asked for at most
    + 1.5 dB; measured with this model on these 64 symbols it is 10.61 dB before and 7.98 dB = threshold + 0.98 dB after (PAPR at 1e-4: 9.36 -> 7.39 dB,
    mean power 0.9898, MER on the carriers the error may reach 29.9 dB), so the bound held here is the measured value + 0.3 dB = + 1.28 dB.  At 1x
    oversampling the same figure is 9.69 dB = + 2.69 dB: oversampling is part of the block."""
    md, iq, power, A, out, ctr = case
    before = cr.interpolated_peak_db(md, iq, power).max()
    after = cr.interpolated_peak_db(md, out, power).max()
    out1, _ = cr.run(md, iq, A, iterations=4, os=1)
    after1 = cr.interpolated_peak_db(md, out1, power).max()
    print(f"\nhighest 8x-interpolated peak: before {before:.2f} dB, after {after:.2f} dB = threshold + {after - PAPR_DB:.2f} dB; at os 1 {after1:.2f} dB; "
          f"PAPR at 1e-4 {cr.papr_db(iq, 1e-4):.2f} -> {cr.papr_db(out, 1e-4):.2f} dB; mean power {np.mean(np.abs(out) ** 2) / power:.4f}")
    assert before > PAPR_DB + 3.0
    assert after <= PAPR_DB + 0.98 + 0.3
    assert after1 > after + 0.5, "oversampling is what holds the interpolated peak down"


def test_pass_through_cases(case):
    md, iq, power, A, _, _ = case
    iq = iq[:3 * md.symbol].copy()
    out, ctr = cr.run(md, iq, A, iterations=0)
    assert (out == iq).all() and ctr["symbols"] == 3 and ctr["symbols_clipped"] == 0 and ctr["peak_power_in"] == 0.0
    out, ctr = cr.run(md, iq, 10 * A)
    assert (out == iq).all() and ctr["symbols_clipped"] == 0 and ctr["samples_over"] == 0 and ctr["peak_power_in"] > 0
    iq[md.symbol + 5] = np.nan
    out, ctr = cr.run(md, iq, A)
    assert ctr["symbols_nonfinite"] == 1 and ctr["symbols_clipped"] == 2
    for l in (0, 2):                                                      # its neighbours are worked on as ever
        assert (out[l * md.symbol:(l + 1) * md.symbol] == cr.run_symbol(md, iq[l * md.symbol:(l + 1) * md.symbol], l, A, 4, 2, 3)).all()
    sl = slice(md.symbol, 2 * md.symbol)
    assert (out[sl].view(np.float64) == iq[sl].astype(np.complex128).view(np.float64))[~np.isnan(out[sl].view(np.float64))].all() and np.isnan(out[md.symbol + 5])
