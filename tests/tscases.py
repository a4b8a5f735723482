"""Transport streams for the analyser's tests, from a seed: a structured stream (several PIDs at given shares with correct counters, a PCR PID at constant
rate, null packets, AF-only packets, PUSI, scrambling bits, random-access flags), named faults injected at given positions, and a stream of random bytes.

A stream is an [n][188] uint8 array.  The structured stream's PCRs are computed from the packet index: pcr(i) = (pcr0 + i tpp) mod 2^33 300, tpp ticks of
27 MHz per packet, so the stream's rate is 188 8 27e6 / tpp bits per second exactly."""
import numpy as np

PCR_MOD = (1 << 33) * 300
NULL_PID = 0x1FFF
PCR_PID = 0x100
PIDS = (0x000, 0x020, 0x100, 0x101, 0x102, 0x1FFF)
SHARES = (0.02, 0.02, 0.56, 0.12, 0.08, 0.20)
TPP = 8000                       # 27 MHz ticks per packet: 5.076 Mbit/s
PCR_GAP = 32                     # packets between two PCRs at least: 256,000 ticks = 9.5 ms


def rate(tpp=TPP):
    return 188 * 8 * 27e6 / tpp


def pid_of(p):
    return ((int(p[1]) & 0x1f) << 8) | int(p[2])


def cc_of(p):
    return int(p[3]) & 15


def set_cc(p, cc):
    p[3] = (int(p[3]) & 0xf0) | (cc & 15)


def get_pcr(p):
    b = [int(x) for x in p[:12]]
    return 300 * (b[6] << 25 | b[7] << 17 | b[8] << 9 | b[9] << 1 | b[10] >> 7) + ((b[10] & 1) << 8 | b[11])


def set_pcr(p, pcr):
    pcr %= PCR_MOD
    base, ext = pcr // 300, pcr % 300
    p[6], p[7], p[8], p[9] = (base >> 25) & 255, (base >> 17) & 255, (base >> 9) & 255, (base >> 1) & 255
    p[10] = ((base & 1) << 7) | 0x7e | (ext >> 8)
    p[11] = ext & 255


def has_pcr(p):
    return (int(p[3]) >> 5) & 1 and 7 <= int(p[4]) <= 183 - ((int(p[3]) >> 4) & 1) and (int(p[5]) >> 4) & 1


def is_plain(p):
    """a packet of payload only"""
    return (int(p[3]) >> 4) & 3 == 1


def structured(n, seed=1, pcr_pid=PCR_PID, tpp=TPP, pcr0=123456789, pids=PIDS, shares=SHARES):
    rs = np.random.RandomState(seed)
    pk = rs.randint(0, 256, size=(n, 188)).astype(np.uint8)
    which = rs.choice(len(pids), size=n, p=shares)
    kind = rs.rand(n)
    pusi = rs.rand(n) < 0.1
    tsc = rs.choice([0, 0, 0, 0, 2, 3], size=n)
    afl_some = rs.randint(1, 21, size=n)
    cc = {p: int(rs.randint(0, 16)) for p in pids}
    last_pcr = None
    for i in range(n):
        pid = pids[which[i]]
        flags = 0x40 if kind[i] < 0.02 or 0.05 <= kind[i] < 0.07 else 0
        if pid == pcr_pid and (last_pcr is None or i - last_pcr >= PCR_GAP):
            afc, afl, flags, last_pcr = 3, 7, flags | 0x10, i
        elif kind[i] < 0.05:
            afc, afl = 2, 183                       # AF only
        elif kind[i] < 0.10:
            afc, afl = 3, int(afl_some[i])
        else:
            afc, afl = 1, None
        if afc & 1:
            cc[pid] = (cc[pid] + 1) & 15
        p = pk[i]
        p[0], p[1], p[2], p[3] = 0x47, (int(pusi[i]) << 6) | (pid >> 8), pid & 255, (int(tsc[i]) << 6) | (afc << 4) | cc[pid]
        if afl is not None:
            p[4], p[5] = afl, flags
            if flags & 0x10:
                set_pcr(p, pcr0 + i * tpp)
    return pk


def find(pk, pid, start, want=is_plain):
    """the position of the first packet of `pid` at or behind `start` that `want` accepts"""
    for i in range(start, len(pk)):
        if pid_of(pk[i]) == pid and want(pk[i]):
            return i
    raise ValueError("the stream is too short for this fault")


def _members(pk, pid, start):
    return [i for i in range(start, len(pk)) if pid_of(pk[i]) == pid]


# ------------------------------------------------------------------ the named faults: (stream, pid, position) -> a new stream
def drop(pk, pid, at):
    i = find(pk, pid, at)
    return np.delete(pk, i, axis=0)


def duplicate(pk, pid, at, copies=1):
    i = find(pk, pid, at)
    return np.insert(pk, [i + 1] * copies, pk[i], axis=0)


def triple(pk, pid, at):
    return duplicate(pk, pid, at, copies=2)


def swap(pk, pid, at):
    """two plain packets of the PID that follow each other in its sequence change places"""
    m = _members(pk, pid, at)
    for a, b in zip(m, m[1:]):
        if is_plain(pk[a]) and is_plain(pk[b]):
            out = pk.copy()
            out[[a, b]] = pk[[b, a]]
            return out
    raise ValueError("no two plain packets in a row")


def excused_jump(pk, pid, at):
    """the counter jumps by 5 at a packet whose adaptation field sets the discontinuity indicator"""
    out = pk.copy()
    m = _members(out, pid, find(out, pid, at))
    p = out[m[0]]
    p[3], p[4], p[5] = (int(p[3]) & 0xcf) | 0x30, 1, 0x80
    for i in m:
        set_cc(out[i], cc_of(out[i]) + 5)
    return out


def tei(pk, pid, at):
    """an extra packet with the transport error indicator (the PID's own sequence stays whole)"""
    i = find(pk, pid, at)
    out = np.insert(pk, i + 1, pk[i], axis=0)
    out[i + 1][1] |= 0x80
    return out


def bad_sync(pk, pid, at):
    i = find(pk, pid, at)
    out = np.insert(pk, i + 1, pk[i], axis=0)
    out[i + 1][0] = 0x48
    return out


def afc_zero(pk, pid, at):
    """an extra packet with adaptation_field_control 00 and the counter of the packet in front of it"""
    i = find(pk, pid, at)
    out = np.insert(pk, i + 1, pk[i], axis=0)
    out[i + 1][3] &= 0xcf
    return out


def af_184(pk, pid, at):
    out = pk.copy()
    p = out[find(out, pid, at)]
    p[3], p[4] = int(p[3]) | 0x30, 184
    return out


def pcr_flag_short(pk, pid, at):
    out = pk.copy()
    p = out[find(out, pid, at)]
    p[3], p[4], p[5] = int(p[3]) | 0x30, 3, 0x10
    return out


def _pcr_step(pk, pid, at, ticks):
    """every PCR of the PID from the first one at or behind `at` on moves by `ticks`"""
    out = pk.copy()
    for i in _members(out, pid, find(out, pid, at, want=has_pcr)):
        if has_pcr(out[i]):
            set_pcr(out[i], get_pcr(out[i]) + ticks)
    return out


def pcr_gap_50ms(pk, pid, at):
    a = find(pk, pid, at, want=has_pcr)
    prev = max(k for k in _members(pk, pid, 0) if has_pcr(pk[k]) and k < a)
    return _pcr_step(pk, pid, at, 1350000 - (get_pcr(pk[a]) - get_pcr(pk[prev])) % PCR_MOD)


def pcr_gap_150ms(pk, pid, at):
    a = find(pk, pid, at, want=has_pcr)
    prev = max(k for k in _members(pk, pid, 0) if has_pcr(pk[k]) and k < a)
    return _pcr_step(pk, pid, at, 4050000 - (get_pcr(pk[a]) - get_pcr(pk[prev])) % PCR_MOD)


def pcr_backwards(pk, pid, at):
    return _pcr_step(pk, pid, at, -1000000)


# name -> (fault, what the whole stream then reads: totals and sums over the PIDs of the counters in ERROR_COUNTERS; every other one is 0)
FAULTS = {
    "drop": (drop, {"cc_errors": 1}),
    "duplicate": (duplicate, {"duplicates": 1}),
    "triple": (triple, {"duplicates": 1, "cc_errors": 1}),
    "swap": (swap, {"cc_errors": 3}),
    "excused_jump": (excused_jump, {"discontinuity": 1}),
    "tei": (tei, {"transport_errors": 1, "tei": 1}),
    "bad_sync": (bad_sync, {"sync_errors": 1}),
    "afc_zero": (afc_zero, {"afc_reserved": 1}),
    "af_184": (af_184, {"af_length_errors": 1}),
    "pcr_flag_short": (pcr_flag_short, {"af_length_errors": 1}),
    "pcr_gap_50ms": (pcr_gap_50ms, {"pcr_over_40ms": 1}),
    "pcr_gap_150ms": (pcr_gap_150ms, {"pcr_over_100ms": 1}),
    "pcr_backwards": (pcr_backwards, {"pcr_over_100ms": 1}),
}
CONTINUITY_FAULTS = ("drop", "duplicate", "triple", "swap")          # exempt on PID 0x1FFF
ERROR_TOTALS = ("sync_errors", "transport_errors", "afc_reserved", "af_length_errors")
ERROR_COUNTERS = ("tei", "duplicates", "cc_errors", "discontinuity", "pcr_discontinuity_signalled", "pcr_over_100ms", "pcr_over_40ms")


def errors(reading):
    """the non-zero error counters of a reading: totals, and sums over its PIDs"""
    out = {f: int(getattr(reading, f)) for f in ERROR_TOTALS}
    out.update({f: int(reading.pids[f].sum()) for f in ERROR_COUNTERS})
    return {f: v for f, v in out.items() if v}


def wrap_stream(n, seed=1, pcr_pid=PCR_PID):
    """a clean stream whose PCR passes 2^33 300 in its middle"""
    return structured(n, seed, pcr_pid, pcr0=PCR_MOD - (n // 2) * TPP - 17)


def random_stream(n, seed=5, few=False):
    """uniformly random bytes with b0 forced to 0x47 on 15 of 16 packets.  Two random PCRs are never within 100 ms of each other, so on three packets of
    four the PCR's bytes are a clock of TPP ticks per packet with a jitter of up to 60 ms: all of step 8 is then met.  few: the PIDs are 0x1FC0 .. 0x1FFF
    only, so that a short stream has sequences to speak of."""
    rs = np.random.RandomState(seed)
    pk = rs.randint(0, 256, size=(n, 188)).astype(np.uint8)
    pk[rs.randint(0, 16, size=n) != 0, 0] = 0x47
    if few:
        pk[:, 1] |= 0x1f
        pk[:, 2] |= 0xc0
    clocked = np.flatnonzero(rs.randint(0, 4, size=n) != 0)
    jitter = rs.randint(0, 1620000, size=n)
    for i in clocked:
        set_pcr(pk[i], PCR_MOD - 1000 * TPP + i * TPP + int(jitter[i]))
    return pk


def distinct_tile(t, seed=3):
    """t plain packets of t different PIDs in a random order"""
    rs = np.random.RandomState(seed)
    pk = rs.randint(0, 256, size=(t, 188)).astype(np.uint8)
    pids = rs.permutation(8191)[:t]
    pk[:, 0], pk[:, 1], pk[:, 2], pk[:, 3] = 0x47, pids >> 8, pids & 255, 0x10 | rs.randint(0, 16, size=t)
    return pk


def plain(pid, cc, n=1, seed=0):
    """n plain packets of one PID with counters cc, cc + 1, ..."""
    pk = np.random.RandomState(seed + pid).randint(0, 256, size=(n, 188)).astype(np.uint8)
    pk[:, 0], pk[:, 1], pk[:, 2], pk[:, 3] = 0x47, pid >> 8, pid & 255, 0x10 | ((cc + np.arange(n)) & 15)
    return pk


def with_pcr(pid, cc, pcr, seed=0):
    """one packet of payload behind an adaptation field that carries `pcr`"""
    p = plain(pid, cc, 1, seed)
    p[0][3], p[0][4], p[0][5] = 0x30 | (cc & 15), 7, 0x10
    set_pcr(p[0], pcr)
    return p
