"""A literal float32 model of ofdm_sym_acquisition (a helper module, not a test file), written from the reference's statements as oracle/o_acq.c restates them
(peak_detect_process :72-146, ml_sync :148-351, general_work :489-568), one general_work call at a time.  It has no lanes, anchors, centres or Jacobi rounds: what
gr_dvbt_amd/csrc/k_frontend.hpp reaches by five routes is computed here by the one route the reference takes.

  * products x[i] conj(x[i - N]) and energy pairs |x[i]|^2 + |x[i - N]|^2 in float32, every operation rounded on its own (the library is built without contraction);
  * per-lag sums over j ascending in float32, one addition at a time;
  * sqrt, half_rho, the literal peak detector with its persistent average;
  * the consume rule, with the halved consume behind a lost lock;
  * reads: `hist` samples of the stream lie in front of the segment's first one, samples at or beyond `avail` read as zeros, and a tap whose partner x[i - N] lies
    in front of what is in memory is skipped (o_acq.c: `if (ci < -back) continue;`), so a lag at the very left of the stream is an ordinary partial sum.

tests/test_acqref.py pins it on the CPU against o_acq_work_hist driven call by call; tests/test_gpu_acquire.py holds the kernels to it bit for bit."""
import math

import numpy as np

F = np.float32
BACK = 32                                       # O_ACQ_BACK: how far in front of in[0] the restatement looks
RISE, FALL, ALPHA = F(0.8), F(0.9), F(0.9)      # :448
ONE_MINUS_ALPHA = F(1) - ALPHA


def half_rho(snr_db):
    snr = F(10.0 ** (float(F(snr_db)) / 10.0))                       # :390-391
    rho = F(float(snr) / (float(snr) + 1.0))
    return F(float(rho) / 2.0)


def peak_detect(d, avg):
    """peak_detect_process on the float32 values d with the carried average; returns (number of completed peaks, position of the largest -- the first of equals --, avg)"""
    state, peak_index, i, n = 0, 0, 0, len(d)
    peak_val = F(-np.inf)
    peaks = []
    while i < n:
        v = d[i]
        if state == 0:
            if v > avg * RISE:
                state = 1
            else:
                avg = ALPHA * v + ONE_MINUS_ALPHA * avg
                i += 1
        elif v > peak_val:
            peak_val, peak_index = v, i
            avg = ALPHA * v + ONE_MINUS_ALPHA * avg
            i += 1
        elif v > avg * FALL:
            avg = ALPHA * v + ONE_MINUS_ALPHA * avg
            i += 1
        else:
            peaks.append(peak_index)
            state, peak_val = 0, F(-np.inf)
    best = -1
    if peaks:
        best, mx = peaks[0], d[peaks[0]]
        for p in peaks[1:]:
            if d[p] > mx:
                best, mx = p, d[p]
    return len(peaks), best, avg


def decisions(d, avg):
    """the rise (bit 0) and keep (bit 1) test of every sample of a window against the average as the sample meets it.  Every sample updates the average exactly once
    and with the same expression in every state of the detector, so the average in front of sample i is the plain recursion over d[:i] from the carried value."""
    out = np.zeros(len(d), np.uint8)
    for i, v in enumerate(d):
        out[i] = (1 if v > avg * RISE else 0) | (2 if v > avg * FALL else 0)
        avg = ALPHA * v + ONE_MINUS_ALPHA * avg
    return out, avg


class Acq:
    """The acquisition block's members and one general_work call (`work`).  buf: complex64, the stream's samples in memory; the segment (absolute sample 0) begins at
    buf[hist]; avail: samples in memory from the segment's first one on."""

    def __init__(self, N, cp, buf, hist=0, avail=None, snr_db=30.0, avg=0.0):
        self.N, self.cp, self.L = N, cp, N + cp
        self.buf = np.ascontiguousarray(buf, dtype=np.complex64)
        self.hist = int(hist)
        self.avail = len(self.buf) - self.hist if avail is None else int(avail)
        assert 0 <= self.hist and self.hist + self.avail <= len(self.buf)
        self.half_rho = half_rho(snr_db)
        self.avg = F(avg)
        self.initial_acq, self.cp_start = False, 0
        self.last = None                                             # the last ml_sync: dict(stop, lam, gr, gi, npk, pos)

    def _read(self, idx):
        ok = (idx >= -self.hist) & (idx < self.avail)
        x = np.zeros(len(idx), np.complex64)
        x[ok] = self.buf[idx[ok] + self.hist]
        return x

    def metric(self, off, start, stop):
        """gamma (two float32 arrays) and lambda of the lags stop .. start - 1 of the call whose in[0] is absolute sample `off`"""
        N, cp, n = self.N, self.cp, start - stop
        back = min(off + self.hist, BACK)
        m = np.arange(stop - cp + 1, start, dtype=np.int64)          # the samples the lags share
        a, b = self._read(off + m), self._read(off + m - N)
        ax, ay, bx, by = a.real.astype(F), a.imag.astype(F), b.real.astype(F), b.imag.astype(F)
        cr, ci = ax * bx + ay * by, ay * bx - ax * by
        e = (ax * ax + ay * ay) + (bx * bx + by * by)
        dead = (m - N) < -back                                       # the partner lies in front of the stream: the tap is skipped
        cr[dead], ci[dead], e[dead] = 0, 0, 0
        gr, gi, phi = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        for j in range(cp):                                          # lag stop + k, tap j: sample stop + k - j
            s = slice(cp - 1 - j, cp - 1 - j + n)
            gr += cr[s]
            gi += ci[s]
            phi += e[s]
        lam = np.sqrt(gr * gr + gi * gi) - phi * self.half_rho
        assert gr.dtype == gi.dtype == lam.dtype == F
        return gr, gi, lam

    def ml_sync(self, off, start, stop):
        gr, gi, lam = self.metric(off, start, stop)
        npk, pos, self.avg = peak_detect(lam, self.avg)
        self.last = {"stop": stop, "lam": lam, "gr": gr, "gi": gi, "npk": npk, "pos": pos, "avg_after": self.avg}
        if npk:
            self.cp_start = pos + stop
        return npk

    def work(self, off):
        """one call with in[0] at absolute sample `off`; returns dict(sync_start, consumed, out, cp_start, gamma (float32 pair at the peak), init / trk: the ml_sync records)"""
        N, cp, L = self.N, self.cp, self.L
        r = {"sync_start": 0, "out": 0, "consumed": L, "init": None, "trk": None, "gamma": None}
        if not self.initial_acq:
            self.initial_acq = self.ml_sync(off, 2 * N + cp - 1, N + cp - 1) > 0
            r["sync_start"], r["init"] = 1, self.last
        if self.initial_acq:
            cur = self.cp_start
            found = self.ml_sync(off, cur + 8, cur - 8)
            r["trk"] = self.last
            if found:
                r["out"] = 1
                r["gamma"] = (self.last["gr"][self.last["pos"]], self.last["gi"][self.last["pos"]])
            else:                                                    # freq_timeout 0: the lock is dropped at once, the call consumes half
                self.initial_acq = False
                r["consumed"] = L // 2
        r["cp_start"] = self.cp_start
        return r


def eps64(g):
    return math.atan2(float(g[1]), float(g[0]))


def run_period(N, cp, buf, nsamples, hist=0, avail=None, snr_db=30.0, init_tries=4, carry=None):
    """One lock period as the segment path sees it: `init_tries` windows for the initial search, call k at sample k (N + cp), tracking until the lock is lost or the
    calls end.  Returns what the kernels leave: status, call0, cp_start0, n_symbols, avg, avg_lost, the initial windows' metric, per symbol cp_start, sw, gamma at the
    peak and the 16 lags examined."""
    L = N + cp
    ncalls = (nsamples - (2 * N + cp + 16)) // L + 1
    a = Acq(N, cp, buf, hist, nsamples if avail is None else avail, snr_db, 0.0 if carry is None else carry)
    out = {"carry": F(0.0 if carry is None else carry), "ncalls": ncalls, "status": 1, "call0": 0, "cp_start0": 0, "n_symbols": 0, "init": [], "sym": [], "lost_trk": None}
    tries = min(ncalls, init_tries)
    call = 0
    while call < tries:
        r = a.work(call * L)
        out["init"].append(r["init"])
        if r["init"]["npk"]:
            break
        call += 1
    else:
        out["avg"] = out["avg_lost"] = a.avg
        return out
    i0 = r["init"]
    out.update(status=0, call0=call, cp_start0=i0["pos"] + N + cp - 1, gamma_init=(i0["gr"][i0["pos"]], i0["gi"][i0["pos"]]))
    out["avg"] = out["avg_lost"] = i0["avg_after"]               # d_avg behind the initial search; avg_lost stays that unless the lock is lost
    prev = out["cp_start0"]
    while True:
        t = r["trk"]
        if not r["out"]:
            out["status"] |= 2
            out["lost_trk"], out["avg_lost"] = t, t["avg_after"]
            break
        out["sym"].append({"cp_start": r["cp_start"], "sw": prev - L, "gamma": r["gamma"], "lag0": t["stop"], "lam": t["lam"], "gr": t["gr"], "gi": t["gi"]})
        prev = r["cp_start"]
        call += 1
        if call >= ncalls:
            break
        r = a.work(call * L)
    out["n_symbols"] = len(out["sym"])
    return out


def literal_phase(N, cp, eps_init, cp_start0, cp_start, eps):
    """The reference's float phase accumulator over the tracked calls (ml_sync :285-313, o_acq.c's advance_phase): one float addition per sample, the increment switching at
    step nextpos of a call when that lies inside it.  eps: the float32 estimate of every call.  Returns the float32 phase at every call's entry."""
    L = N + cp
    pi, twopi = F(math.pi), F(2.0 * math.pi)
    phase, phaseinc, nextinc, nextpos = F(0), 0.0, (-1.0 / N) * float(F(eps_init)), cp_start0 - L
    entry = []
    for c, e in zip(cp_start, eps):
        entry.append(phase)
        for i in range(L):
            if i == nextpos:
                phaseinc = nextinc
            phase = F(float(phase) + phaseinc)
            while phase > pi:
                phase = phase - twopi
            while phase < -pi:
                phase = phase + twopi
        nextinc, nextpos = (-1.0 / N) * float(F(e)), int(c) - L
    return np.array(entry, F)
