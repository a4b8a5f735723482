"""dvbt_fft (gr_dvbt_amd.Block("fft", N, forward, 1)) at every size it accepts, 64 .. 8192, in both directions.

- unit impulses: every input index for N <= 512, 64 seeded ones and 0, N/2 - 1, N/2, N - 1 above; each output is the tone of txref.single_bin_output.
  These pin the digit reversal (fft_pos_of_bin) and the half-spectrum shift for every radix sequence of fft_dif_lds;
- Gaussian items against numpy complex128: the maximum error within 1e-5 of the peak, the relative RMS error within RMS_K times that of a complex64
  FFT on the CPU (torch);
- 1, 2, 3 and 4097 items in a call, and device calls at item offsets: every item is transformed alone;
- FFT(IFFT(x)) = N x.
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

RMS_K = 6.0                 # measured on MI355X: 2.2 - 3.4 up to N = 2048, 4.1 - 4.3 at 4096 and 8192
SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    return gr_dvbt_amd


def _fft(g, x, N, forward):
    b = g.Block("fft", N, int(forward), 1)
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1, N)
    out = np.zeros_like(x)
    r, cons, _ = b.work(len(x), len(x), x, out)
    b.close()
    assert (r, cons) == (len(x), len(x))
    return out


@pytest.mark.parametrize("forward", [1, 0])
@pytest.mark.parametrize("N", SIZES)
def test_single_bins(g, N, forward):
    if N <= 512:
        bins = np.arange(N)
    else:
        bins = np.unique(np.concatenate([np.random.RandomState(N + forward).randint(0, N, 64), [0, N // 2 - 1, N // 2, N - 1]]))
    x = np.zeros((len(bins), N), np.complex64)
    x[np.arange(len(bins)), bins] = 1
    out = _fft(g, x, N, forward)
    ref = np.stack([txref.single_bin_output(N, int(b), bool(forward)) for b in bins])
    err = np.abs(out - ref).max(axis=1)
    # an ordinary float32 FFT is ~1e-6 off here; the wrong bin, sign or shift is off by O(1)
    assert err.max() <= 2e-5, (N, forward, int(bins[err.argmax()]), float(err.max()))


@pytest.mark.parametrize("forward", [1, 0])
@pytest.mark.parametrize("N", SIZES)
def test_gaussian_items_against_float64(g, N, forward):
    rng = np.random.RandomState(7 * N + forward)
    x = (rng.randn(6, N) + 1j * rng.randn(6, N)).astype(np.complex64)
    out = _fft(g, x, N, forward)
    ref = txref.fft64(x, forward)
    assert np.abs(out - ref).max() <= 1e-5 * np.abs(ref).max()
    r_gpu = txref.rel_rms(out, ref)
    r_f32 = txref.rel_rms(txref.fft32(x, forward), ref)
    print(f"\nrms fft fwd={forward} N={N} gpu={r_gpu:.3e} f32={r_f32:.3e} ratio={r_gpu / r_f32:.2f}")
    assert r_gpu <= RMS_K * r_f32, (N, forward, r_gpu, r_f32)


@pytest.mark.parametrize("N", SIZES)
def test_round_trip(g, N):
    rng = np.random.RandomState(N)
    x = (rng.randn(3, N) + 1j * rng.randn(3, N)).astype(np.complex64)
    back = _fft(g, _fft(g, x, N, 0), N, 1)
    assert np.abs(back - N * x).max() <= 1e-5 * np.abs(N * x).max()


@pytest.mark.skipif(torch is None, reason="needs torch")
@pytest.mark.parametrize("N,forward", [(64, 1), (64, 0), (128, 0), (2048, 1), (8192, 0)])
def test_items_do_not_interact(g, N, forward):
    rng = np.random.RandomState(N + 3 * forward)
    M = 4097 if N == 64 else 37
    x = (rng.randn(M, N) + 1j * rng.randn(M, N)).astype(np.complex64)
    whole = _fft(g, x, N, forward)
    ref = txref.fft64(x, forward)
    assert np.abs(whole - ref).max() <= 1e-5 * np.abs(ref).max()
    # 1, 2 and 3 items in a call: the same bits as in the big call (every item is one workgroup's own transform)
    for a, n in ((0, 1), (1, 2), (M - 3, 3)):
        assert _fft(g, x[a:a + n], N, forward).tobytes() == whole[a:a + n].tobytes()
    # device calls at item offsets into one buffer
    b = g.Block("fft", N, forward, 1)
    din = torch.from_numpy(x.view(np.float32).copy()).cuda()
    dout = torch.full((M * N * 2,), float("nan"), dtype=torch.float32, device="cuda")
    pos = 0
    for n in (1, 2, 3, 5, M - 11):
        r, cons, _ = b.work_device(n, n, din.data_ptr() + pos * N * 8, dout.data_ptr() + pos * N * 8)
        assert (r, cons) == (n, n)
        pos += n
    assert pos == M
    torch.cuda.synchronize()
    b.close()
    assert dout.cpu().numpy().view(np.complex64).reshape(M, N).tobytes() == whole.tobytes()
