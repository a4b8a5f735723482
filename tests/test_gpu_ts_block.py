"""The GPU transport-stream analyser (dvbt_ts_*, gr_dvbt_amd.TsAnalyser) against its model tests/tsref.py.

Every accumulated quantity is a 64-bit integer, so the totals and every field of every PID's entry are compared for EQUALITY: there is no tolerance in this
file except the 1e-9 on a float64 bit rate.  tests/test_ts_model.py shows that the streams used here move every counter.  T = DVBT_TS_TILE is where the
device cuts its work; the cases under "tile edges" put a PID's packets on both sides of such a cut.

Not tested here: the cap of 2^40 packets per stream (DVBT_ERR_CAPACITY).  It is one comparison in front of the enqueue (ts_check_call), beside the ones
that are tested.
"""
import ctypes as C

import numpy as np
import pytest

import tscases as tc
import tsref

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

T = 1024
LENGTHS = (0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)
X, Y, FILL = 0x0777, 0x0778, 0x0050


@pytest.fixture(scope="module")
def g():
    import gr_dvbt_amd
    assert gr_dvbt_amd.device_count() > 0, "GPU tests need a GPU; the product path has no fallback"
    L = gr_dvbt_amd.lib()
    L.dvbt_device_malloc.restype = C.c_void_p
    L.dvbt_device_malloc.argtypes = [C.c_size_t]
    L.dvbt_device_free.argtypes = [C.c_void_p]
    L.dvbt_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    assert gr_dvbt_amd.TS_TILE == T, "this file's cases stand on the implementation's tile edges"
    return gr_dvbt_amd


@pytest.fixture(scope="module")
def streams():
    """name -> (packets, the model's reading of every prefix in LENGTHS); computed once, never written"""
    out = {}
    for name, pk in (("random, 64 PIDs", tc.random_stream(max(LENGTHS), few=True)), ("random", tc.random_stream(max(LENGTHS), seed=6)),
                     ("structured", tc.structured(max(LENGTHS), seed=2))):
        pk.setflags(write=False)
        out[name] = (pk, {n: tsref.analyse(pk[:n]) for n in LENGTHS})
    return out


class Dev:
    """bytes on the device at `shift` bytes behind an allocation's start, 0xA5 around them (the library's own allocator and blocking copies)"""
    PAD = 256

    def __init__(self, g, pk, shift=0):
        self.L = g.lib()
        self.data = np.ascontiguousarray(pk, dtype=np.uint8).reshape(-1)
        self.image = np.full(len(self.data) + 2 * self.PAD, 0xA5, np.uint8)
        self.image[self.PAD + shift:self.PAD + shift + len(self.data)] = self.data
        self.raw = self.L.dvbt_device_malloc(len(self.image))
        assert self.raw and self.raw % 16 == 0
        assert self.L.dvbt_copy_to_device(C.c_void_p(self.raw), self.image.ctypes.data_as(C.c_void_p), len(self.image)) == 0
        self.base = self.raw + self.PAD + shift

    def at(self, packet):
        return self.base + 188 * packet

    def unchanged(self):
        back = np.zeros_like(self.image)
        assert self.L.dvbt_copy_to_host(back.ctypes.data_as(C.c_void_p), C.c_void_p(self.raw), len(back)) == 0
        return np.array_equal(back, self.image)

    def free(self):
        self.L.dvbt_device_free(C.c_void_p(self.raw))


def bits(reading):
    return tuple(int(getattr(reading, f)) for f in tsref.TOTALS), np.asarray(reading.pids).tobytes()


def check(a, pk, what=""):
    """the handle's reading equals the model's of pk, field by field"""
    got, want = a.read(), pk if isinstance(pk, tsref.Result) else tsref.analyse(pk)
    d = tsref.diff(got, want)
    assert not d, (what, d)
    assert bits(got) == bits(want), what
    return got


# ------------------------------------------------------------------ 1. against the model, exactly
@pytest.mark.parametrize("name", ["random, 64 PIDs", "random", "structured"])
def test_every_length_equals_the_model(g, streams, name):
    pk, want = streams[name]
    a = g.TsAnalyser(max_packets=4 * T)
    for n in LENGTHS:
        a.reset()
        a.push(pk[:n])
        got = check(a, want[n], n)
        assert got.packets_pushed == n
    a.close()


def test_all_8192_pids_at_once(g):
    """2^17 random packets: every PID occurs, a tile holds about 900 runs of its 1024 packets"""
    pk = tc.random_stream(1 << 17)
    a = g.TsAnalyser()
    a.push(pk)
    got = check(a, pk)
    assert got.pids_seen == 8192 and int(got.pids["pcr_pairs"].sum()) > 0 and int(got.pids["duplicates"].sum()) > 0
    a.close()


# ------------------------------------------------------------------ 2. tile edges
def lay(n, placed):
    """n packets: `placed` {position: packet} among plain packets of PID FILL whose counter runs on correctly"""
    pk = np.zeros((n, 188), np.uint8)
    free = np.array([i for i in range(n) if i not in placed], dtype=np.int64)
    pk[free] = tc.plain(FILL, 3, len(free))
    for pos, p in placed.items():
        pk[pos] = np.asarray(p).reshape(188)
    return pk


def px(cc, pid=X, tei=False):
    p = tc.plain(pid, cc)[0]
    if tei:
        p[1] |= 0x80
    return p


def bumped(pk, by):
    """the same packets with every counter `by` further"""
    out = pk.copy()
    out[:, 3] = (out[:, 3] & 0xf0) | ((out[:, 3] + by) & 15)
    return out


EDGES = {
    "tiles 0 and 2 only, in order": (lay(3 * T, {5: px(3), 2 * T + 7: px(4)}), {}),
    "tiles 0 and 2 only, a gap": (lay(3 * T, {5: px(3), 2 * T + 7: px(6)}), {"cc_errors": 1}),
    "two packets astride an edge, a duplicate": (lay(2 * T, {T - 1: px(9), T: px(9)}), {"duplicates": 1}),
    "two packets astride an edge, a drop": (lay(2 * T, {T - 1: px(9), T: px(11)}), {"cc_errors": 1}),
    "a triple as 1 | 2": (lay(2 * T, {T - 1: px(15), T: px(15), T + 1: px(15)}), {"duplicates": 1, "cc_errors": 1}),
    "a triple as 2 | 1": (lay(2 * T, {T - 2: px(15), T - 1: px(15), T: px(15)}), {"duplicates": 1, "cc_errors": 1}),
    "a run of 1 behind a carried same": (lay(3 * T, {T - 9: px(4), T - 2: px(4), T + 30: px(4), 2 * T + 1: px(5)}), {"duplicates": 1, "cc_errors": 1}),
    "a run of 2 behind a carried same": (lay(2 * T, {T - 9: px(4), T - 2: px(4), T + 30: px(4), T + 31: px(4)}), {"duplicates": 1, "cc_errors": 2}),
    "a run of 1 then a duplicate": (lay(3 * T, {T - 2: px(4), T + 30: px(5), 2 * T + 1: px(5), 2 * T + 2: px(5)}), {"duplicates": 1, "cc_errors": 1}),
    "a PCR pair astride an edge": (lay(2 * T, {T - 3: tc.with_pcr(X, 1, 1000)[0], T + 4: tc.with_pcr(X, 2, 501000)[0]}), {}),
    "a PCR pair over two empty tiles": (lay(4 * T, {5: tc.with_pcr(X, 1, tc.PCR_MOD - 7)[0], 3 * T + 2: tc.with_pcr(X, 2, 2000000)[0]}), {"pcr_over_40ms": 1}),
    "a PCR pair over an edge, too long": (lay(2 * T, {T - 1: tc.with_pcr(X, 1, 1000)[0], T: tc.with_pcr(X, 2, 2701001)[0]}), {"pcr_over_100ms": 1}),
    "one PID only": (np.concatenate([tc.plain(X, 2, T), tc.plain(X, 2 + T, 700), tc.plain(X, 2 + T + 699, T + 3 - 700)]), {"duplicates": 1}),
    "T distinct PIDs, twice": (np.concatenate([tc.distinct_tile(T), bumped(tc.distinct_tile(T), 3), tc.plain(tc.NULL_PID, 0, 5)]), {"cc_errors": T}),
    "a TEI packet between two tiles' members": (lay(2 * T, {T - 1: px(1), T: px(7, tei=True), T + 1: px(2)}), {"transport_errors": 1, "tei": 1}),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_tile_edges(g, name):
    pk, expect = EDGES[name]
    want = tsref.analyse(pk)
    assert tc.errors(want) == expect, "the case is what its name says"
    a = g.TsAnalyser(max_packets=4 * T)
    a.push(pk)
    check(a, want, name)
    if name.startswith("a PCR pair"):
        assert int(want.entry(X)["pcr"]) == 2
    a.close()


def test_more_tiles_than_the_carry_takes_at_once(g):
    """the carry takes a batch's tiles 64 at a time: 66 tiles and 3 packets of 64 busy PIDs, with a PID in tiles 0 and 65 only (a triple over that distance),
    one whose PCR pair lies astride tile 63 | 64 and one whose only run of one member is the last of tile 63"""
    n = 66 * T + 3
    pk = tc.random_stream(n, seed=11, few=True)
    for pos, p in {5: px(3), 65 * T + 7: px(3), 65 * T + 9: px(3), 64 * T - 2: tc.with_pcr(Y, 1, 1000)[0], 64 * T + 2: tc.with_pcr(Y, 2, 1200000)[0],
                   62 * T + 1: px(8, 0x0779), 64 * T - 1: px(8, 0x0779), 64 * T: px(8, 0x0779)}.items():
        pk[pos] = p
    want = tsref.analyse(pk)
    assert (int(want.entry(X)["duplicates"]), int(want.entry(X)["cc_errors"]), int(want.entry(Y)["pcr_over_40ms"])) == (1, 1, 1)
    assert (int(want.entry(0x0779)["duplicates"]), int(want.entry(0x0779)["cc_errors"])) == (1, 1)
    a = g.TsAnalyser(max_packets=n)
    a.push(pk)
    check(a, want)
    a.reset()
    a.push(pk[:64 * T - 1])
    a.push(pk[64 * T - 1:])
    check(a, want, "cut in front of the last packet of tile 63")
    a.close()


# ------------------------------------------------------------------ 3. a stream cut into calls
def test_a_stream_cut_anywhere_gives_the_same_bytes(g, streams):
    assert torch is not None
    pk, models = streams["random, 64 PIDs"]
    n = len(pk)
    want = bits(models[n])
    a = g.TsAnalyser(max_packets=4 * T)
    a.push(pk)
    assert bits(a.read()) == want
    for cut in range(41):
        a.reset()
        a.push(pk[:cut])
        a.push(pk[cut:])
        assert bits(a.read()) == want, cut
    for size in (1, T - 1, T + 1):
        a.reset()
        for pos in range(0, n, size):
            a.push(pk[pos:pos + size])
        assert bits(a.read()) == want, size
    a.close()
    # batches inside one call
    b = g.TsAnalyser(max_packets=T + 1)
    b.push(pk)
    assert bits(b.read()) == want
    # push and push_device in turn, on two streams
    dev = Dev(g, pk)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    b.reset()
    pos = 0
    for i, size in enumerate((700, 1, T, 0, T + 3, 40, n - 2 * T - 744)):
        if i % 2 == 0:
            b.push_device(dev.at(pos), size, stream=(s1 if i % 4 == 0 else s2).cuda_stream)
        else:
            b.push(pk[pos:pos + size])
        pos += size
    assert pos == n and bits(b.read()) == want
    # reset: the state after create
    b.reset()
    empty = b.read()
    assert bits(empty) == bits(tsref.analyse(pk[:0])) and len(empty.pids) == 0
    b.push_device(dev.at(0), n)
    assert bits(b.read()) == want
    b.close()
    dev.free()


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 5])
def test_any_byte_alignment_and_nothing_written(g, streams, shift):
    pk, models = streams["random, 64 PIDs"]
    n = 2 * T + 1
    dev = Dev(g, pk[:n], shift=shift)
    assert dev.base % 4 == shift % 4
    a = g.TsAnalyser(max_packets=4 * T)
    a.push_device(dev.base, n)
    check(a, models[n], shift)
    assert dev.unchanged(), "the packets and the 0xA5 on both sides are as they were"
    a.close()
    dev.free()


# ------------------------------------------------------------------ 4. refusals on a live handle
def test_a_refused_call_leaves_the_stream_where_it_was(g, streams):
    pk, models = streams["structured"]
    a = g.TsAnalyser(max_packets=4 * T)
    a.push(pk[:T + 1])
    before = bits(a.read())
    assert before == bits(models[T + 1])
    L = g.lib()
    assert L.dvbt_ts_push(a.h, None, 2) == -1 and L.dvbt_ts_push_device(a.h, None, 2, None) == -1
    assert bits(a.read()) == before
    assert L.dvbt_ts_push(a.h, None, 0) == 0 and L.dvbt_ts_push_device(a.h, None, 0, None) == 0, "no packets: accepted, nothing added"
    res, n = g.TsResult(), C.c_size_t()
    seen = len(a.read().pids)
    small = np.zeros(seen - 1, g.TS_PID_DTYPE)
    assert L.dvbt_ts_read(a.h, C.byref(res), small.ctypes.data_as(C.c_void_p), seen - 1, C.byref(n)) == -4
    assert L.dvbt_ts_read(a.h, C.byref(res), None, 0, C.byref(n)) == 0 and n.value == seen == res.pids_seen and res.packets_pushed == T + 1
    assert bits(a.read()) == before and bits(a.read()) == before, "a read does not disturb the accumulation"
    a.push(pk[T + 1:])
    check(a, models[len(pk)])
    a.close()


def test_handles_destroyed_with_work_queued(g, streams):
    pk, models = streams["random"]
    dev = Dev(g, pk)
    for i in range(50):
        a = g.TsAnalyser(max_packets=2 * T)
        a.push_device(dev.at(0), len(pk))
        if i == 49:
            check(a, models[len(pk)])
        a.close()
    assert dev.unchanged()
    dev.free()


# ------------------------------------------------------------------ 5. behind the receiver
SUPERFRAMES = 2        # the receiver delivers from the first superframe start it has seen announced


@pytest.fixture(scope="module")
def sent(g):
    """one packet more than two superframes of 2k QAM16 1/2 take, so that a stream with one packet removed is as long as the clean one"""
    d = g.get_dims(g.QAM16, g.C1_2, g.T2k)
    npk = SUPERFRAMES * 272 * d.payload_length * d.m * d.cr_k // d.cr_n // 8 // 204
    pk = tc.structured(npk + 1, seed=12)
    pk.setflags(write=False)
    return pk


def _loopback(g, ts):
    tx = g.Tx(g.QAM16, g.C1_2, g.T2k, scale=float(np.float32(0.0022097087) * np.float32(0.0022097087)))
    iq = tx.run(ts)
    tx.close()
    iq = np.concatenate([np.zeros(1000, np.complex64), iq, np.zeros(3 * 2048, np.complex64)])
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=len(iq), taps=True)
    rx.run(iq)
    return rx


def test_behind_the_receiver(g, sent):
    rx = _loopback(g, sent[:-1])
    tap = np.asarray(rx.tap(g.TAP_TS)).reshape(-1)
    n = len(tap) // 188
    assert n >= 400, "the case is meant to deliver most of a superframe's 504 packets"
    out = tap[:n * 188].reshape(n, 188)
    a = g.TsAnalyser.from_rx(rx)
    got = check(a, out)
    assert got.packets_pushed == n and tc.errors(got) == {}
    assert (got.sync_errors, got.transport_errors, int(got.pids["cc_errors"].sum())) == (0, 0, 0)
    rate = got.ts_bitrate(tc.PCR_PID)
    print(f"\n{n} packets behind the receiver, {got.pids_seen} PIDs, TS rate by PCR {rate:.3f} bit/s against {tc.rate():.3f}")
    assert abs(rate - tc.rate()) <= 1e-9 * tc.rate()
    a.close()
    # the same stream with one plain packet of PID 0x101 taken out of what the receiver delivers
    first = next(i for i in range(len(sent)) if np.array_equal(sent[i], out[0]))
    assert np.array_equal(sent[first:first + n], out), "the receiver delivers the packets sent"
    victim = tc.find(sent, 0x101, first + n // 2)
    assert victim < first + n - 40
    rx2 = _loopback(g, np.delete(sent, victim, axis=0))
    b = g.TsAnalyser.from_rx(rx2)
    hurt = b.read()
    assert tc.errors(hurt) == {"cc_errors": 1} and int(hurt.entry(0x101)["cc_errors"]) == 1
    assert hurt.tr101290()["continuity_count_error"] == 1
    b.close()
    rx.close()
    rx2.close()


def test_from_rx_needs_a_segment(g):
    rx = g.Rx(g.QAM16, g.C1_2, g.T2k, max_samples=1 << 16)
    with pytest.raises(g.DvbtError, match="has not run"):
        g.TsAnalyser.from_rx(rx)
    a = g.TsAnalyser(max_packets=T)
    with pytest.raises(g.DvbtError, match="has not run"):
        a.push_rx(rx)
    with pytest.raises(g.DvbtError, match="whole packets"):
        a.push(np.zeros(189, np.uint8))
    a.close()
    rx.close()
