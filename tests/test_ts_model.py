"""The transport-stream analyser's model (tests/tsref.py) and generator (tests/tscases.py) mean what they say.  CPU only: the device is compared with
this model for equality in tests/test_gpu_ts_block.py, and these tests show that the comparison there is about something."""
import numpy as np
import pytest

import tscases as tc
import tsref

N = 1500
AT = 700


@pytest.fixture(scope="module")
def clean():
    pk = tc.structured(N)
    pk.setflags(write=False)
    return pk


@pytest.fixture(scope="module")
def clean_null():
    """the same stream with PID 0x1FFF as the PCR PID, for the faults' variants on that PID"""
    pk = tc.structured(N, pcr_pid=tc.NULL_PID)
    pk.setflags(write=False)
    return pk


def test_the_clean_stream_reads_all_zero(clean, clean_null):
    for pk, pcr_pid in ((clean, tc.PCR_PID), (clean_null, tc.NULL_PID)):
        r = tsref.analyse(pk)
        assert tc.errors(r) == {}
        assert r.packets_pushed == N and r.pids_seen == len(tc.PIDS)
        e = r.entry(pcr_pid)
        assert e["pcr"] >= 10 and e["pcr_pairs"] == e["pcr"] - 1 and e["sum_dt"] == tc.TPP * e["sum_dp"]
        assert all(r.entry(p)["packets"] > 0 for p in tc.PIDS)
        for f in ("pusi", "scrambled", "payload", "adaptation", "random_access"):
            assert int(r.pids[f].sum()) > 0, f
        assert int((r.pids["packets"] - r.pids["payload"]).sum()) > 0, "AF-only packets are in"


@pytest.mark.parametrize("name", sorted(tc.FAULTS))
def test_a_fault_alone_moves_exactly_its_counter(clean, name):
    fault, expect = tc.FAULTS[name]
    r = tsref.analyse(fault(clean, tc.PCR_PID, AT))
    assert tc.errors(r) == expect
    other = tsref.analyse(fault(clean, 0x101, AT)) if not name.startswith("pcr_gap") and name != "pcr_backwards" else None
    if other is not None:
        assert tc.errors(other) == expect and {k: int(other.entry(0x101)[k]) for k in expect if k in tsref.FIELDS} == {k: v for k, v in expect.items() if k in tsref.FIELDS}


@pytest.mark.parametrize("name", sorted(tc.FAULTS))
def test_the_same_fault_on_pid_0x1fff(clean_null, name):
    """continuity is not evaluated there; everything else is"""
    fault, expect = tc.FAULTS[name]
    r = tsref.analyse(fault(clean_null, tc.NULL_PID, AT))
    assert tc.errors(r) == ({} if name in tc.CONTINUITY_FAULTS else expect)


def test_a_pcr_that_wraps_is_in_order():
    for pcr_pid in (tc.PCR_PID, tc.NULL_PID):
        pk = tc.wrap_stream(N, pcr_pid=pcr_pid)
        pcrs = [tc.get_pcr(p) for p in pk if tc.pid_of(p) == pcr_pid and tc.has_pcr(p)]
        assert any(b < a for a, b in zip(pcrs, pcrs[1:])), "the wrap is in the stream"
        r = tsref.analyse(pk)
        e = r.entry(pcr_pid)
        assert tc.errors(r) == {} and e["pcr_pairs"] == len(pcrs) - 1 and e["sum_dt"] == tc.TPP * e["sum_dp"]


def test_the_random_stream_moves_every_counter():
    pk = tc.random_stream(1 << 17)
    r = tsref.analyse(pk)
    assert r.pids_seen == 8192, "every PID occurs"
    for f in tsref.TOTALS:
        assert getattr(r, f) > 0, f
    for f in tsref.FIELDS:
        assert int(r.pids[f].sum()) > 0, f
    assert int((r.pids["min_dt"] >= 0).sum()) > 0 and int(r.pids["max_dp"].max()) > 0
    hdr = pk[pk[:, 0] == 0x47]
    assert len(np.unique(hdr[:, 3])) == 256 and len(np.unique(hdr[:, 1])) == 256 and len(np.unique(hdr[:, 4])) == 256 and len(np.unique(hdr[:, 5])) == 256
    # and the short one the GPU tests cut into calls
    short = tsref.analyse(tc.random_stream(3 * 1024 + 5, few=True))
    assert short.pids_seen == 64 and short.entry(tc.NULL_PID)["packets"] > 0
    for f in tsref.TOTALS:
        assert getattr(short, f) > 0, f
    for f in tsref.FIELDS:
        assert int(short.pids[f].sum()) > 0, f


def test_two_walks_with_carried_state_equal_one():
    for pk in (tc.random_stream(40, seed=8), tc.triple(tc.structured(38, seed=4), tc.PCR_PID, 10), np.repeat(tc.random_stream(4, seed=9), 10, axis=0)):
        assert len(pk) == 40
        whole = tsref.analyse(pk)
        for cut in range(41):
            a = tsref.analyse(pk[:cut])
            both = tsref.combine(a, tsref.analyse(pk[cut:], start=a.state))
            assert not tsref.diff(both, whole), (cut, tsref.diff(both, whole))
        # and without the state the walks differ somewhere
    pk = tc.triple(tc.structured(38, seed=4), tc.PCR_PID, 10)
    whole = tsref.analyse(pk)
    assert any(tsref.diff(tsref.combine(tsref.analyse(pk[:c]), tsref.analyse(pk[c:])), whole) for c in range(1, 40))


def test_ts_bitrate_is_the_generated_rate(clean):
    import gr_dvbt_amd as g
    r = tsref.analyse(clean)
    reading = g.TsReading(r.totals, r.pids)
    assert reading.ts_bitrate(tc.PCR_PID) == pytest.approx(tc.rate(), rel=4e-16)
    assert np.isnan(reading.ts_bitrate(0x101))
    lo, mean, hi = reading.pcr_interval_ms(tc.PCR_PID)
    assert tc.PCR_GAP * tc.TPP / 27e3 <= lo <= mean <= hi < 40.0
    assert reading.share(tc.NULL_PID) == reading.null_share == r.entry(tc.NULL_PID)["packets"] / N
    assert reading.pid_bitrate(0x101, tc.rate()) == r.entry(0x101)["packets"] / N * tc.rate()
    assert reading.tr101290() == {"sync_byte_error": 0, "continuity_count_error": 0, "transport_error": 0, "PCR_repetition_error": 0,
                                  "PCR_discontinuity_indicator_error": 0}
    bad = tsref.analyse(tc.pcr_gap_150ms(tc.drop(clean, 0x101, AT), tc.PCR_PID, AT))
    t = g.TsReading(bad.totals, bad.pids).tr101290()
    assert (t["continuity_count_error"], t["PCR_repetition_error"], t["PCR_discontinuity_indicator_error"]) == (1, 1, 1)


def test_ts_align_finds_the_first_packet(clean):
    import gr_dvbt_amd as g
    body = clean[:8].copy()
    body[:, 1:] = 0                                  # no 0x47 but the sync bytes
    rs = np.random.RandomState(2)
    for junk in range(188):
        lead = rs.randint(0, 256, size=junk).astype(np.uint8)
        lead[lead == 0x47] = 0x46
        assert g.ts_align(np.concatenate([lead, body.reshape(-1)])) == junk
        assert g.ts_align(bytes(lead) + body.tobytes()) == junk
    with pytest.raises(g.DvbtError):
        g.ts_align(np.zeros(4 * 188, np.uint8))
    with pytest.raises(g.DvbtError):
        g.ts_align(clean[:4])
