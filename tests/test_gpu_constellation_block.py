"""The GPU constellation analyser (dvbt_constellation_*, gr_dvbt_amd.Constellation) against its model tests/constref.py.

Every accumulated quantity is an integer and the model spells out the float32 operations in front of the quantisation, so every output -- the density, the
point moments, the carrier sums, the counts -- is compared for EQUALITY: there is no tolerance in this file except where a figure of another instrument
(rx.quality()) is met.  tests/test_constellation_model.py shows that the comparison would see an fma contraction.

Not tested here: the cap of 2^33 cells per stream (DVBT_ERR_CAPACITY).  Reaching it takes 64 GB of input; it is one comparison in front of the enqueue
(constellation_check_call), beside the ones that are tested.
"""
import ctypes as C

import numpy as np
import pytest

import constref as cr

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

GRID_IDS = [f"c{c}h{h}" for c, h in cr.GRIDS]
ROW_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1512, 6048)
ROW_COUNTS = (0, 1, 2, 3, 31, 32, 33, 100)


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    L = gr_dvbt_amd.lib()
    L.dvbt_device_malloc.restype = C.c_void_p
    L.dvbt_device_malloc.argtypes = [C.c_size_t]
    L.dvbt_device_free.argtypes = [C.c_void_p]
    L.dvbt_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    assert gr_dvbt_amd.Constellation is not None
    return gr_dvbt_amd


class Dev:
    """rows on the device (the library's own allocator and blocking copies: ordered with work on the default stream)"""

    def __init__(self, g, x, shift=0):
        self.L = g.lib()
        x = np.ascontiguousarray(x)
        self.rowbytes = x.dtype.itemsize * x.shape[1]
        self.raw = self.L.dvbt_device_malloc(x.nbytes + 64)
        assert self.raw and self.raw % 16 == 0
        self.base = self.raw + shift                    # shift 8: rows that are 8-byte aligned only
        if x.nbytes:
            assert self.L.dvbt_copy_to_device(C.c_void_p(self.base), x.ctypes.data_as(C.c_void_p), x.nbytes) == 0

    def at(self, row):
        return self.base + self.rowbytes * row

    def free(self):
        self.L.dvbt_device_free(C.c_void_p(self.raw))


def _diff(got, want):
    """where two readings differ, in words"""
    out = []
    for name in ("rows_pushed", "cells", "nonfinite", "clipped", "levels", "alpha", "span"):
        if getattr(got, name) != getattr(want, name):
            out.append(f"{name}: {getattr(got, name)} != {getattr(want, name)}")
    if not np.array_equal(got.hist, want.hist):
        out.append(f"hist: {int((got.hist != want.hist).sum())} bins differ")
    for arr in ("points", "carriers"):
        a, b = getattr(got, arr), getattr(want, arr)
        for f in a.dtype.names:
            if not np.array_equal(a[f], b[f]):
                out.append(f"{arr}.{f}: {int((a[f] != b[f]).sum())} entries differ")
    return out


# ------------------------------------------------------------------ 1. against the model, exactly
@pytest.mark.parametrize("P", ROW_LENGTHS)
@pytest.mark.parametrize("c,h", cr.GRIDS, ids=GRID_IDS)
def test_every_output_equals_the_model(g, c, h, P):
    cells = cr.stream(c, h, max(ROW_COUNTS), P)
    assert cells.size <= 10 ** 6
    a = g.Constellation(c, h, row_length=P)
    for n in ROW_COUNTS:
        a.reset()
        a.push(cells[:n])
        want = cr.analyse(cells[:n], c, h)
        if n == max(ROW_COUNTS) and P >= 63:
            assert want.nonfinite > 0 and want.clipped > 0, "the special cells are in"
        got = a.read()
        assert not _diff(got, want), (n, _diff(got, want))
        assert cr.bits_of(got) == cr.bits_of(want)
    a.close()


def test_rows_that_are_only_8_byte_aligned(g):
    """an even row length on a base that is 8 mod 16: the one-cell loads"""
    cells = cr.stream(2, 0, 33, 256)
    dev = Dev(g, cells, shift=8)
    a = g.Constellation(g.QAM64, row_length=256)
    a.push_device(dev.at(0), 33)
    assert cr.bits_of(a.read()) == cr.bits_of(cr.analyse(cells, 2, 0))
    a.close()
    dev.free()


# ------------------------------------------------------------------ 2. a stream cut into calls
SPLITS = {"one call": (100,), "1, 0, 99": (1, 0, 99), "33, 33, 34": (33, 33, 34), "row by row": (1,) * 100}


def test_a_stream_cut_into_calls_gives_the_same_bytes(g):
    assert torch is not None
    c, h, P, n = 2, 0, 257, 100
    cells = cr.stream(c, h, n, P)
    other = cr.stream(1, 3, n, P, seed=7)
    want, want_other = cr.bits_of(cr.analyse(cells, c, h)), cr.bits_of(cr.analyse(other, 1, 3))
    dev, dev2 = Dev(g, cells), Dev(g, other)
    a = g.Constellation(c, h, row_length=P)
    for name, cuts in SPLITS.items():
        for entry in ("host", "device"):
            a.reset()
            pos = 0
            for i, k in enumerate(cuts):
                if entry == "host":
                    a.push(cells[pos:pos + k])
                else:
                    a.push_device(dev.at(pos), k)
                pos += k
                if i == 0 and len(cuts) > 1:
                    part = a.read()                        # a read between the pushes
                    assert cr.bits_of(part) == cr.bits_of(cr.analyse(cells[:pos], c, h)), (name, entry)
            assert cr.bits_of(a.read()) == want, (name, entry)
            assert cr.bits_of(a.read()) == want, "a read does not disturb the accumulation"
    # two handles fed alternately on two streams, each changing its stream with every call
    b = g.Constellation(1, 3, row_length=P)
    a.reset()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pos = 0
    for i, k in enumerate((33, 33, 34)):
        sa, sb = (s1, s2) if i % 2 == 0 else (s2, s1)
        a.push_device(dev.at(pos), k, stream=sa.cuda_stream)
        b.push_device(dev2.at(pos), k, stream=sb.cuda_stream)
        pos += k
    assert cr.bits_of(a.read()) == want and cr.bits_of(b.read()) == want_other
    a.close()
    b.close()
    dev.free()
    dev2.free()


# ------------------------------------------------------------------ 3. contention
@pytest.mark.parametrize("kind", ["one bin", "two adjacent bins"])
def test_identical_cells_are_all_counted(g, kind):
    """64 rows of 6048 cells on one point and in one bin (387,072 of them), or in two adjacent bins: what a narrow or lost LDS counter fails"""
    c, h, P, n = 2, 0, 6048, 64
    L, H, alpha, S, inv_d = cr.grid(c, h)
    pt = cr.ideal_cells(c, h)[L * L - 1]
    cells = np.full((n, P), pt, np.complex64)
    if kind == "two adjacent bins":
        step = np.float32(2.0 * S / cr.G / np.float64(inv_d))              # one bin's width
        cells[:, 1::2] = pt + step
    want = cr.analyse(cells, c, h)
    assert int((want.hist > 0).sum()) == (1 if kind == "one bin" else 2) and int((want.points["n"] > 0).sum()) == 1
    a = g.Constellation(c, h, row_length=P)
    a.push(cells)
    got = a.read()
    assert int(got.hist.sum()) == n * P == 387072 and int(got.hist.max()) == int(want.hist.max())
    assert int(got.points["n"][L * L - 1]) == n * P
    assert cr.bits_of(got) == cr.bits_of(want), _diff(got, want)
    a.close()


def test_a_workgroups_counter_holds_more_than_16_bits(g):
    """8192 identical rows of 6048 identical cells, made on the device: the launch spreads a call over about two workgroups per CU, so that only a call of
    this size gives one workgroup's LDS counter more than 2^16 (here about 97,000 on a device of 256 CUs).  Every row is the same, so the model of one row
    times 8192 is the expectation."""
    assert torch is not None
    c, h, P, n = 2, 0, 6048, 8192
    L = cr.grid(c, h)[0]
    pt = cr.ideal_cells(c, h)[L + 2] * np.complex64(1.01)
    one = cr.analyse(np.full((1, P), pt, np.complex64), c, h)
    rows = torch.full((n, P), complex(pt), dtype=torch.complex64, device="cuda:0")
    torch.cuda.synchronize()
    a = g.Constellation(c, h, row_length=P)
    a.push_device(rows.data_ptr(), n)
    got = a.read()
    assert (got.rows_pushed, got.cells, got.nonfinite, got.clipped) == (n, n * P, 0, 0)
    assert np.array_equal(got.hist, one.hist * np.uint64(n)) and int(got.hist.max()) == n * P
    for arr in ("points", "carriers"):
        for f in getattr(got, arr).dtype.names:
            assert np.array_equal(getattr(got, arr)[f], getattr(one, arr)[f] * n), (arr, f)
    assert int(got.points["sum_re2"][L + 2]) > 0
    a.close()
    del rows


# ------------------------------------------------------------------ 4. refusals on a live handle
def test_a_refused_call_leaves_the_accumulation_as_it_was(g):
    c, h, P = 1, 0, 65
    cells = cr.stream(c, h, 33, P)
    a = g.Constellation(c, h, row_length=P)
    a.push(cells[:6])
    before = cr.bits_of(a.read())
    L = g.lib()
    rows = np.zeros((3, P + 1), np.complex64)
    ptr = rows.ctypes.data
    refusals = (("null rows", None, 2, -1), ("misaligned rows", C.c_void_p(ptr + 4), 2, -1), ("more than 2^24 rows", C.c_void_p(ptr), (1 << 24) + 1, -1))
    for what, r, n, code in refusals:
        assert L.dvbt_constellation_push(a.h, r, n) == code, what
        assert L.dvbt_constellation_push_device(a.h, r, n, None) == code, what
        assert cr.bits_of(a.read()) == before, what
    assert L.dvbt_constellation_push(a.h, None, 0) == 0 and L.dvbt_constellation_push_device(a.h, None, 0, None) == 0, "no rows: accepted, nothing added"
    res = g.ConstellationResult()
    small_p, small_c = np.zeros(15, g.POINT_DTYPE), np.zeros(P - 1, g.CARRIER_DTYPE)
    assert L.dvbt_constellation_read(a.h, C.byref(res), None, small_p.ctypes.data_as(C.c_void_p), 15, None, 0) == -4
    assert L.dvbt_constellation_read(a.h, C.byref(res), None, None, 0, small_c.ctypes.data_as(C.c_void_p), P - 1) == -4
    assert L.dvbt_constellation_read(a.h, C.byref(res), None, None, 0, None, 0) == 0
    assert (res.rows_pushed, res.cells, res.points, res.levels, res.alpha, res.span) == (6, 6 * P, 16, 4, 1, 4)
    assert cr.bits_of(a.read()) == before
    a.push(cells[6:])
    assert cr.bits_of(a.read()) == cr.bits_of(cr.analyse(cells, c, h))
    a.close()


# ------------------------------------------------------------------ 5. end to end on the device
SUPERFRAMES = 2        # the receiver delivers from the first superframe start it has seen announced: of two superframes sent it equalises one (272 rows), of one none


@pytest.fixture(scope="module")
def baseband(g):
    """2k QAM16 1/2 from the modulator, behind 1000 zeros and in front of 3 N (the sounder's test stream)"""
    scale = float(np.float32(0.0022097087) * np.float32(0.0022097087))
    tx = g.Tx(g.QAM16, g.C1_2, g.T2k, scale=scale)
    d = tx.dims
    npk = SUPERFRAMES * 272 * d.payload_length * d.m * d.cr_k // d.cr_n // 8 // 204
    ts = np.random.RandomState(9 * 1000003).randint(0, 256, size=(npk, 188)).astype(np.uint8)
    ts[:, 0] = 0x47
    iq = tx.run(ts)
    tx.close()
    assert len(iq) == SUPERFRAMES * 272 * (d.fft_length + d.cp_length)
    out = np.concatenate([np.zeros(1000, np.complex64), iq, np.zeros(3 * 2048, np.complex64)])
    out.setflags(write=False)
    return out


def _through(g, baseband, echoes):
    """the baseband through the channel block (20 dB AWGN, seed 11) and the receiver; (rx, report)"""
    body = baseband[1000:len(baseband) - 3 * 2048]
    sigma = g.Channel.sigma(20.0, float(np.mean(np.abs(body.astype(np.complex128)) ** 2)))
    ch = g.Channel(echoes=echoes, fft_length=2048, noise_sigma=sigma, seed=11)
    iq = ch.run(baseband)
    ch.close()
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=len(iq), snr_db=20.0, taps=True, quality=True)     # (told the channel's SNR, the acquisition holds its lock)
    return rx, rx.run(iq)


def test_end_to_end_behind_the_receiver(g, baseband):
    rx, rep = _through(g, baseband, ((19, 0.3),))
    assert rep.n_lock_periods == 1 and rep.n_out_symbols >= 270, "the case is meant to hold the lock and deliver a superframe of equalised rows"
    eq = rx.tap(g.TAP_EQ)
    assert eq.shape == (rep.n_out_symbols, 1512)
    a = g.Constellation.from_rx(rx)
    got = a.read()
    want = cr.analyse(eq, g.QAM16, 0)
    assert not _diff(got, want), _diff(got, want)
    assert cr.bits_of(got) == cr.bits_of(want)
    q = rx.quality()
    print(f"\nMER {got.mer_db:.4f} dB, rx.quality() {q.mer_db:.4f} dB over {rep.n_out_symbols} rows; STE {got.ste()}, suppression {got.carrier_suppression_db:.1f} dB")
    assert q.mer_carriers == got.cells and abs(got.mer_db - q.mer_db) <= 0.01
    # the echo's ripple across the carriers, against the same chain without the echo
    flat_rx, flat_rep = _through(g, baseband, ())
    flat = g.Constellation.from_rx(flat_rx).read()
    spread, spread_flat = float(np.std(got.mer_per_carrier_db)), float(np.std(flat.mer_per_carrier_db))
    print(f"spread of the MER per carrier: {spread:.3f} dB behind the echo, {spread_flat:.3f} dB without")
    assert np.isfinite(got.mer_per_carrier_db).all() and np.isfinite(flat.mer_per_carrier_db).all()
    assert flat_rep.n_lock_periods == 1 and flat_rep.n_out_symbols >= 270 and spread > spread_flat
    # first_row, and a second push on the same handle
    a.reset()
    a.push_rx(rx, first_row=3)
    assert cr.bits_of(a.read()) == cr.bits_of(cr.analyse(eq[3:], g.QAM16, 0))
    a.close()
    rx.close()
    flat_rx.close()


def test_from_rx_needs_a_buffer_and_a_segment(g, baseband):
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=len(baseband), taps=True)
    with pytest.raises(g.DvbtError, match="has not run"):
        g.Constellation.from_rx(rx)
    rx.close()
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=len(baseband))
    rx.run(baseband)
    with pytest.raises(g.DvbtError, match="taps=True or quality=True"):
        g.Constellation.from_rx(rx)
    other = g.Constellation(g.QAM64, row_length=1512)
    with pytest.raises(g.DvbtError):
        other.push_rx(rx)
    other.close()
    rx.close()
