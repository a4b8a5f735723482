"""tests/acqref.py (the literal float32 model that tests/test_gpu_acquire.py holds the acquisition kernels to) against oracle/o_acq.c, both driven one general_work call
at a time over the same streams: where every call begins, what it consumes, whether it delivers a symbol, the lock periods and every cp_start must be identical;
epsilon (atan2f there, float64 atan2 of the model's own correlation here) within the bound the GPU test uses.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import acqcases
import acqref


def drive_oracle(po, c, iq, snr_db=30.0):
    """o_chain.c's loop over o_acq_work_hist: rows (pos, sync_start, consumed, produced, cp_start, epsilon)"""
    L = po.lib()
    L.o_acq_new.argtypes = [C.POINTER(po.Cfg), C.c_float]
    L.o_acq_free.argtypes = [C.c_void_p]
    L.o_acq_set_avail.argtypes = [C.c_void_p, C.c_longlong]
    L.o_acq_work_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong] + [C.c_void_p] * 5
    iq = np.ascontiguousarray(iq, np.complex64)
    out = np.zeros(c.N, np.complex64)
    a = L.o_acq_new(C.byref(c), snr_db)
    rows, pos = [], 0
    cons, sync, cps, eps = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
    while pos + 2 * c.N + c.cp + 16 <= len(iq):
        L.o_acq_set_avail(a, len(iq) - pos)
        prod = L.o_acq_work_hist(a, iq[pos:].ctypes.data_as(C.c_void_p), pos, out.ctypes.data_as(C.c_void_p), C.byref(cons), C.byref(sync), C.byref(cps), C.byref(eps))
        rows.append((pos, sync.value, cons.value, prod, cps.value, eps.value))
        pos += cons.value
    L.o_acq_free(a)
    return rows


def drive_model(c, iq, snr_db=30.0):
    a = acqref.Acq(c.N, c.cp, iq, 0, len(iq), snr_db)
    rows, pos = [], 0
    while pos + 2 * c.N + c.cp + 16 <= len(iq):
        r = a.work(pos)
        rows.append((pos, r["sync_start"], r["consumed"], r["out"], r["cp_start"], r["gamma"]))
        pos += r["consumed"]
    return rows


def periods(rows):
    """[(call position, symbols)] of the lock periods: a period begins at a call that searched and delivered"""
    out = []
    for pos, sync, _, prod, _, _ in rows:
        if sync and prod:
            out.append([pos, 0])
        if prod:
            out[-1][1] += 1
    return [tuple(p) for p in out]


def compare(po, c, iq, snr_db=30.0):
    ro, rm = drive_oracle(po, c, iq, snr_db), drive_model(c, iq, snr_db)
    assert [r[:5] for r in ro] == [r[:5] for r in rm]
    got = np.array([r[5] for r in ro if r[3]], np.float32)
    gam = [r[5] for r in rm if r[3]]
    worst, yard, bound = acqcases.eps_check(got, gam)
    print(f"\n{len(ro)} calls, periods {periods(ro)[:6]}, epsilon: worst {worst:.3e} rad, float32 arctan2 {yard:.3e}, bound {bound:.3e}")
    assert worst <= bound
    return ro


@pytest.mark.parametrize("lead_in", acqcases.LEAD_INS_ONE_PERIOD)
def test_lead_in_one_period(po, lead_in):
    """a stream that begins within 8 samples of a symbol start: the first tracking window reaches in front of the stream, the taps there are skipped, the lock holds"""
    c, iq = acqcases.clean_stream(po, lead_in)
    ro = compare(po, c, iq)
    assert periods(ro) == [(0, 323)]
    assert all(r[4] == 2111 + lead_in for r in ro if r[3])


@pytest.mark.parametrize("lead_in", acqcases.LEAD_INS_TWO_PERIODS)
def test_lead_in_two_periods(po, lead_in):
    """the symbol start lies at or behind the first window's last lag: the search locks onto what it finds there, call 0 delivers one symbol, call 1 finds no peak and
    consumes half a call, and the search of the call at 3,168 = 2,112 + 1,056 begins the period that holds the other 322 symbols.  (With other packets the first lock
    can fail in call 0 already: one period of 323 symbols from 1,056 then.  These are the figures of this module's stream, make_ts(300, 17), from the oracle.)"""
    c, iq = acqcases.clean_stream(po, lead_in)
    ro = compare(po, c, iq)
    assert periods(ro) == [(0, 1), (3168, 322)]


def test_8k_guard_1_4(po):
    c = po.cfg(po.QPSK, po.C1_2, po.T8k, po.G1_4)
    iq = po.tx(c, po.make_ts(60, 3), lead_in=300, tail=3 * c.N)
    ro = compare(po, c, iq)
    assert len(periods(ro)) == 1 and periods(ro)[0][1] >= 10


def test_two_echoes_and_offset(po):
    c, iq = acqcases.clean_stream(po, 500, npk=100)
    iq = po.channel(iq, c.N, cfo=0.37, echoes=((9, 0.5 + 0.2j), (41, -0.25j)), snr_db=25.0, seed=8, ref_span=(1000, 101000))
    ro = compare(po, c, iq)
    assert sum(n for _, n in periods(ro)) >= 90                      # (the reference's detector drops this lock a few times: all the better)


def test_noise_that_loses_the_lock(po):
    c, iq = acqcases.clean_stream(po, 500)
    iq = po.channel(iq, c.N, snr_db=acqcases.LOSSY_SNR_DB, seed=11)
    ro = compare(po, c, iq, snr_db=acqcases.LOSSY_SNR_DB)
    assert len(periods(ro)) >= 3, periods(ro)
