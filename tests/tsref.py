"""The transport-stream analyser's model: the specification in include/dvbt_hip.h (dvbt_ts_*), steps 1 to 9, as a plain sequential walk with a dict per PID.

analyse(packets) walks a stream from its first packet.  analyse(packets, start=r.state) continues behind an earlier walk `r`: the state is what the
specification says a PID's next packet can depend on -- (cc, pay, same) of its last member and its last PCR with index -- plus the packet count, and
combine(a, b) adds the two walks' counts.  Nothing here is vectorised: it is meant to be read beside the header."""
import copy

import numpy as np

FIELDS = ("pid", "packets", "pusi", "scrambled", "payload", "adaptation", "discontinuity", "random_access", "pcr", "tei", "duplicates", "cc_errors",
          "first", "last", "pcr_pairs", "pcr_discontinuity_signalled", "pcr_over_100ms", "pcr_over_40ms", "sum_dt", "sum_dp", "min_dt", "max_dt", "max_dp")
PID_DTYPE = np.dtype([(f, np.int64) for f in FIELDS])
TOTALS = ("packets_pushed", "sync_errors", "transport_errors", "afc_reserved", "af_length_errors", "pids_seen")
PCR_MOD = (1 << 33) * 300
NULL_PID = 0x1FFF


def _entry(pid):
    e = dict.fromkeys(FIELDS, 0)
    e["pid"], e["first"], e["min_dt"] = pid, -1, -1
    return e


class State:
    """what a walk hands to the walk behind it"""

    def __init__(self):
        self.i = 0                 # the next packet's index
        self.member = {}           # pid -> (cc, pay, same) of its last member
        self.pcr = {}              # pid -> (pcr, i) of its last member with a PCR


class Result:
    def __init__(self, totals, entries, state):
        self.totals, self.entries, self.state = totals, entries, state
        seen = sorted(p for p, e in entries.items() if e["packets"] + e["tei"] > 0)
        self.totals["pids_seen"] = len(seen)
        self.pids = np.array([tuple(entries[p][f] for f in FIELDS) for p in seen], dtype=PID_DTYPE).reshape(-1)
        for f in TOTALS:
            setattr(self, f, self.totals[f])

    def entry(self, pid):
        return self.entries.get(pid, _entry(pid))


def as_packets(data):
    d = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    assert len(d) % 188 == 0, "whole packets"
    return d.reshape(-1, 188)


def analyse(data, start=None):
    st = copy.deepcopy(start) if start is not None else State()
    tot = dict.fromkeys(TOTALS, 0)
    ent = {}
    for b in as_packets(data).tolist():
        i = st.i
        st.i += 1
        tot["packets_pushed"] += 1
        # 1
        if b[0] != 0x47:
            tot["sync_errors"] += 1
            continue
        # 2
        tei, pusi, pid = b[1] >> 7, (b[1] >> 6) & 1, ((b[1] & 0x1f) << 8) | b[2]
        tsc, afc, cc = b[3] >> 6, (b[3] >> 4) & 3, b[3] & 15
        pay, af = afc & 1, afc >> 1
        e = ent.setdefault(pid, _entry(pid))
        # 3
        if tei:
            tot["transport_errors"] += 1
            e["tei"] += 1
            continue
        # 4
        e["packets"] += 1
        e["pusi"] += pusi
        e["scrambled"] += 1 if tsc != 0 else 0
        e["payload"] += pay
        e["adaptation"] += af
        if e["first"] < 0:
            e["first"] = i
        e["last"] = i
        # 5
        if afc == 0:
            tot["afc_reserved"] += 1
        # 6
        di = rai = pf = 0
        pcr = None
        if af:
            afl = b[4]
            if afl > 183 - pay:
                tot["af_length_errors"] += 1
            elif afl >= 1:
                di, rai, pf = b[5] >> 7, (b[5] >> 6) & 1, (b[5] >> 4) & 1
                e["discontinuity"] += di
                e["random_access"] += rai
                if pf and afl < 7:
                    tot["af_length_errors"] += 1
                elif pf:
                    base = b[6] << 25 | b[7] << 17 | b[8] << 9 | b[9] << 1 | b[10] >> 7
                    ext = (b[10] & 1) << 8 | b[11]
                    pcr = 300 * base + ext
                    e["pcr"] += 1
        # 7
        j = st.member.get(pid)
        same_i = 0
        if j is not None:
            cc_j, pay_j, same_j = j
            same_i = int(bool(pay and pay_j and cc == cc_j and not di))
            if pid != NULL_PID and not di:
                if cc == ((cc_j + pay) & 15):
                    pass
                elif same_i and not same_j:
                    e["duplicates"] += 1
                else:
                    e["cc_errors"] += 1
        st.member[pid] = (cc, pay, same_i)
        # 8
        if pcr is not None:
            a = st.pcr.get(pid)
            if a is not None:
                if di:
                    e["pcr_discontinuity_signalled"] += 1
                else:
                    dt, dp = (pcr - a[0]) % PCR_MOD, i - a[1]
                    if dt > 2700000:
                        e["pcr_over_100ms"] += 1
                    else:
                        e["pcr_pairs"] += 1
                        e["sum_dt"] += dt
                        e["sum_dp"] += dp
                        e["min_dt"] = dt if e["min_dt"] < 0 else min(e["min_dt"], dt)
                        e["max_dt"] = max(e["max_dt"], dt)
                        e["max_dp"] = max(e["max_dp"], dp)
                        if dt > 1080000:
                            e["pcr_over_40ms"] += 1
            st.pcr[pid] = (pcr, i)
    return Result(tot, ent, st)


def combine(a, b):
    """the counts of walk `a` and of the walk `b` that continued it"""
    tot = {f: a.totals[f] + b.totals[f] for f in TOTALS}
    ent = copy.deepcopy(a.entries)
    for pid, y in b.entries.items():
        x = ent.setdefault(pid, _entry(pid))
        for f in FIELDS:
            if f in ("pid", "first", "last", "min_dt", "max_dt", "max_dp"):
                continue
            x[f] += y[f]
        if y["packets"]:
            x["first"] = y["first"] if x["first"] < 0 else x["first"]
            x["last"] = y["last"]
        if y["min_dt"] >= 0:
            x["min_dt"] = y["min_dt"] if x["min_dt"] < 0 else min(x["min_dt"], y["min_dt"])
        x["max_dt"], x["max_dp"] = max(x["max_dt"], y["max_dt"]), max(x["max_dp"], y["max_dp"])
    return Result(tot, ent, b.state)


def diff(got, want):
    """where two readings (anything with the totals as attributes and `pids`) differ, in words"""
    out = [f"{f}: {getattr(got, f)} != {getattr(want, f)}" for f in TOTALS if int(getattr(got, f)) != int(getattr(want, f))]
    g, w = np.asarray(got.pids), np.asarray(want.pids)
    if len(g) != len(w) or not np.array_equal(g["pid"], w["pid"]):
        return out + [f"the PIDs seen differ: {len(g)} against {len(w)}"]
    for f in FIELDS:
        bad = np.flatnonzero(g[f] != w[f])
        if len(bad):
            k = bad[0]
            out.append(f"{f}: {len(bad)} PIDs differ, first pid {int(g['pid'][k])}: {int(g[f][k])} != {int(w[f][k])}")
    return out
