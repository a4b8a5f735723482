"""The kernels of gr_dvbt_amd/csrc/k_drift.hpp ALONE (dvbt_debug_drift: a test hook of the library), where tests/test_gpu_channel.py reaches them only through a whole
receiver and a tolerance on the equalised carriers far downstream.  The reference is the literal accumulator restated in tests/drift/drift_host.cpp (one float addition
per sample, ofdm_sym_acquisition_impl.cc:285-309), compiled here as tests/test_drift_model.py compiles it; its --dump mode runs nothing of the closed form.

Segment path (drift_prep / drift_exact / drift_round<0,1,2> / drift_seq / drift_table, the launch sequence of enqueue itself): every deviation within 1e-5 rad of the
literal one -- the bound of tests/test_drift_model.py, a factor 13 under the 1.35e-4 rad that the 1e-3 tolerance of the equalised-carrier tap corresponds to -- at the
edges of the scans (256 runs per workgroup in drift_round, 1, 2, 3 calls per thread in drift_exact), at every guard interval's call length, at the benchmark's 17,680
calls, and where the increment is a few float ulps under estimates that jitter: there three rounds of the fixed point leave up to 1e-3 rad and the kernels have to
notice and take the recurrence over the calls.  What the model does not cover is refused on the device: flags[1] = 0, delta untouched.
Block path (drift_table_entry): any increments from the literal accumulator's own entry phase; calls with an increment under DRIFT_MIN_INC take the exact line by
design and are only required to be finite."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import gr_dvbt_amd as g

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                                     # rad
MIN_INC = 2.0 * 2.384185791015625e-07          # DRIFT_MIN_INC of k_drift_math.hpp
EPS_FILE = os.path.join(ROOT, "tests", "golden", "drift_eps_8k_echo_cfo.txt")


@pytest.fixture(scope="module")
def lit(tmp_path_factory):
    """literal(N, cp, nsym, eps, jitter, seed, *options) -> the calls and what the literal accumulator makes of them; every case is computed once"""
    d = tmp_path_factory.mktemp("drift")
    exe = str(d / "drift_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "drift", "drift_host.cpp")])

    @functools.lru_cache(maxsize=None)
    def literal(N, cp, nsym, eps, jitter, seed=1, *opts):
        f = str(d / "case.bin")
        subprocess.check_output([exe, str(N), str(cp), str(nsym), repr(eps), repr(jitter), str(seed), *opts, "--dump", f])
        raw = open(f, "rb").read()
        os.remove(f)
        hdr = np.frombuffer(raw, np.int32, 4)
        assert tuple(hdr[:3]) == (N, cp, nsym)
        nb, o = int(hdr[3]), 16
        out = {"N": N, "cp": cp, "nsym": nsym, "nb": nb}
        for k, dt, n in (("sw", np.int32, nsym), ("incA", np.float64, nsym), ("incB", np.float64, nsym), ("entry", np.float32, nsym), ("lit", np.float64, nsym * nb)):
            out[k] = np.frombuffer(raw, dt, n, o)
            o += n * np.dtype(dt).itemsize
        assert o == len(raw)
        out["lit"] = out["lit"].reshape(nsym, nb)
        return out
    return literal


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def drift(c, path=0, status=0, flags=(0, 0, 0, 0), nsym=None, **over):
    """dvbt_debug_drift on the calls of c (arrays replaced by `over`); returns (delta [nsym][N / 32] as float32, the four flag words, milliseconds)"""
    L = g.lib()
    L.dvbt_debug_drift.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    n = c["nsym"] if nsym is None else nsym
    a = {k: np.ascontiguousarray(over.get(k, c[k])) for k in ("sw", "incA", "incB", "entry")}
    assert a["sw"].dtype == np.int32 and a["incA"].dtype == a["incB"].dtype == np.float64 and a["entry"].dtype == np.float32
    delta = np.zeros((max(n, 1), c["nb"]), np.float32)
    fl = np.array(flags, np.int32)
    ms = C.c_float(0)
    g.binding._chk(L.dvbt_debug_drift(c["N"], c["cp"], n, _p(a["sw"]), _p(a["incA"]), _p(a["incB"]), _p(a["entry"]), status, path, _p(delta), _p(fl), C.byref(ms)))
    return delta[:n], tuple(int(x) for x in fl), ms.value


def check_segment(c, name, recurrence):
    """recurrence: whether the period is one on which the fixed point's three rounds do not settle (flags[3]: drift_seq_kernel then walks the calls)"""
    d, fl, ms = drift(c)
    err = np.abs(d.astype(np.float64) - c["lit"])
    err = np.where(np.isnan(err), np.inf, err)                       # a deviation the kernels did not write
    worst = err.max()
    print(f"\n[{name}] {c['nsym']} calls, wander {np.abs(c['lit']).max():.2e}, worst error {worst:.2e} rad at call {int(err.max(axis=1).argmax())} (bound {TOL:.0e}), "
          f"{'recurrence' if fl[3] else 'fixed point'}, {ms:.3f} ms")
    assert fl == (0, 1, 1 if c["incB"][0] < 0 else 0, 1 if recurrence else 0), fl
    assert np.isfinite(d).all()
    assert worst <= TOL
    return d, ms


# ------------------------------------------------------------------------------------------------ segment path
@pytest.mark.parametrize("eps", [2.3247788, -1.2566])
@pytest.mark.parametrize("nsym", [2, 3, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_scan_edges(lit, nsym, eps):
    """around the 256 runs of a workgroup of drift_round and the change from 1 to 2 to 3 calls per thread of drift_exact"""
    check_segment(lit(2048, 64, nsym, eps, 1e-6), f"2k/64 eps {eps}", False)


# the last column: whether the recurrence is taken (the CPU replay of tests/drift/drift_host.cpp says so on stderr: the rounds 4.5e-10, 2.2e-7, 0 and 2.6e-4 rad apart)
SHAPES = [
    (8192, 2048, 300, 1.0, 1e-4, False),
    (2048, 512, 700, -0.8, 1e-4, False),
    (8192, 256, 544, 0.0044, 1e-6, False),     # the small-increment edge: 2.25 ulp of the coarsest binade
    (8192, 256, 544, -0.0057, 1e-4, True),     # 2.9 ulp: the step jumps between 2 and 3 ulp
]


@pytest.mark.parametrize("N,cp,nsym,eps,jitter,recurrence", SHAPES, ids=[f"{s[0]}/{s[1]} {s[2]} calls eps {s[3]}" for s in SHAPES])
def test_other_shapes(lit, N, cp, nsym, eps, jitter, recurrence):
    check_segment(lit(N, cp, nsym, eps, jitter), f"{N}/{cp} eps {eps} jitter {jitter}", recurrence)


@pytest.mark.parametrize("eps,jitter", [(2.3247788, 1e-6), (-2.32, 0.02)])
def test_the_benchmarks_size(lit, eps, jitter):
    """17,680 calls of 8k.  The second case's estimates jitter enough that three rounds leave 1.2e-5 rad; it takes the recurrence.  The launch sequence's time is printed
    for a second call as well (the first one loads the kernels)."""
    c = lit(8192, 256, 17680, eps, jitter)
    d, _ = check_segment(c, f"8k/256 eps {eps} jitter {jitter}", jitter > 1e-3)
    d2, _, ms = drift(c)
    print(f"[8k/256 eps {eps} jitter {jitter}] launch sequence, second call: {ms:.3f} ms")
    assert d.tobytes() == d2.tobytes()


JITTER = [
    (8192, 256, 544, 0.02, 3e-3, 1),
    (8192, 256, 3000, 0.01, 1e-3, 1),
    (8192, 256, 600, 0.006, 5e-4, 1),
    (8192, 256, 600, 0.006, 5e-4, 2),
    (2048, 64, 3000, 0.0012, 5e-5, 1),
    (2048, 64, 1100, -0.02, 3e-3, 1),
    (8192, 256, 17680, -2.32, 0.02, 1),
]


@pytest.mark.parametrize("N,cp,nsym,eps,jitter,seed", JITTER, ids=[f"{s[0]}/{s[1]} {s[2]} calls eps {s[3]} jitter {s[4]} seed {s[5]}" for s in JITTER])
def test_increments_of_a_few_ulps_under_jitter(lit, N, cp, nsym, eps, jitter, seed):
    """the step rint(inc / ulp) * ulp of a region jumps from call to call: the fixed point's three rounds are up to 9.7e-4 rad away (tests/test_drift_model.py)"""
    check_segment(lit(N, cp, nsym, eps, jitter, seed), f"{N}/{cp} eps {eps} jitter {jitter} seed {seed}", True)


def test_the_oracles_epsilon_on_an_echo_with_a_small_offset(lit):
    """8k QAM64 7/8, an echo at 0.3 cp of -20 dB and a carrier offset of 0.003 subcarriers: epsilon as the oracle estimates it (tests/golden/make_drift_golden.py)"""
    check_segment(lit(8192, 256, 544, 0.0, 0.0, 1, "--eps-file", EPS_FILE), "8k/256 oracle epsilon, echo + cfo 0.003", True)


def _base(lit):
    return lit(2048, 64, 300, 2.3247788, 1e-6)


def _applied(c):
    """the flag words behind a period the model covers"""
    return (0, 1, 1 if c["incB"][0] < 0 else 0, 0)


def _refusals(c):
    L = c["N"] + c["cp"]

    def put(key, i, v):
        a = c[key].copy()
        a[i] = v
        return a
    return [
        ("increments of both signs", dict(incB=put("incB", 5, -c["incB"][5]), incA=put("incA", 6, -c["incB"][5]))),
        ("one increment below DRIFT_MIN_INC", dict(incB=put("incB", 7, np.copysign(0.5 * MIN_INC, c["incB"][7])), incA=put("incA", 8, np.copysign(0.5 * MIN_INC, c["incB"][7])))),
        ("one increment of zero", dict(incB=put("incB", 299, 0.0))),
        ("a switch at -1", dict(sw=put("sw", 3, -1))),
        ("a switch at N + cp", dict(sw=put("sw", 298, L))),
        ("a carried increment in front of the first switch", dict(incA=put("incA", 0, c["incB"][0]))),
        ("a single call", dict(nsym=1)),
        ("no call", dict(nsym=0)),
        ("initial acquisition failed", dict(status=1)),
        ("initial acquisition failed, further bits set", dict(status=7)),
    ]


def _poisoned(d):
    return bool((d.view(np.uint32) == 0xFFFFFFFF).all())


@pytest.mark.parametrize("k", range(10))
def test_what_the_model_does_not_cover_is_refused(lit, k):
    c = _base(lit)
    name, how = _refusals(c)[k]
    before = (0, 1, 1 - _applied(c)[2], 1)      # what an applied period of the other sign that took the recurrence leaves: drift_exact_kernel has to clear it
    d, fl, _ = drift(c, flags=before, **how)
    print(f"\n[{name}] flags {before} -> {fl}")
    assert fl[0] == 0 and fl[1] == 0 and fl[3] == 0, name
    if how.get("nsym") == 0:
        assert d.size == 0                       # (nothing to read back: the flag words are the whole answer)
    else:
        assert d.size > 0 and _poisoned(d), name


def test_hand_over_between_periods(lit):
    """a refused period leaves the flag words such that the next period starts clean; the same call twice gives the same bits"""
    c = _base(lit)
    fresh, fl0, _ = drift(c)
    assert fl0 == _applied(c) and np.isfinite(fresh).all()
    again, fl1, _ = drift(c)
    assert fl1 == fl0 and again.tobytes() == fresh.tobytes()
    for name, how in _refusals(c):
        _, fl, _ = drift(c, flags=fl0, **how)
        assert fl[1] == 0, name
        after, fl2, _ = drift(c, flags=fl)
        assert fl2 == fl0 and after.tobytes() == fresh.tobytes(), name
    # and a period of the other sign behind an applied one
    n = lit(2048, 64, 257, -1.2566, 1e-6)
    a, fla, _ = drift(n)
    b, flb, _ = drift(n, flags=fl0)
    assert fla == flb == _applied(n) and fla[2] != fl0[2] and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ block path
BLOCK = [
    ("8k/256, 600 calls, both signs", (8192, 256, 600, 0.0, 1.0, 1, "--mixed")),
    ("2k/64, 1,100 calls, both signs", (2048, 64, 1100, 0.0, 1.0, 1, "--mixed")),
    ("8k/2048, 300 calls, both signs, one switch outside its call", (8192, 2048, 300, 0.0, 1.0, 1, "--mixed", "--sw-out", "151")),
]


@pytest.mark.parametrize("name,args", BLOCK, ids=[b[0] for b in BLOCK])
def test_block_path_from_the_literal_entry_phase(lit, name, args):
    c = lit(*args)
    assert (c["incB"] > 0).any() and (c["incB"] < 0).any()
    if "--sw-out" in args:
        assert c["sw"][151] >= c["N"] + c["cp"] and abs(c["incA"][151]) >= MIN_INC and abs(c["incB"][151]) >= MIN_INC
    d, fl, ms = drift(c, path=1)
    assert fl[1] == 1
    assert np.isfinite(d).all()                                      # the calls left out below included
    inside = (np.abs(c["incA"]) >= MIN_INC) & (np.abs(c["incB"]) >= MIN_INC)
    out = int((~inside).sum())
    err = np.abs(d.astype(np.float64) - c["lit"]).max(axis=1)
    print(f"\n[block path: {name}] wander {np.abs(c['lit']).max():.2e}, worst error {err[inside].max():.2e} rad (bound {TOL:.0e}) over {int(inside.sum())} calls; "
          f"{out} calls with an increment under DRIFT_MIN_INC left out (worst there {err[~inside].max():.2e}), {ms:.3f} ms")
    assert out < 0.05 * c["nsym"]
    assert err[inside].max() <= TOL


def test_block_path_switch_at_minus_one(lit):
    """a switch position in front of the call: the whole call runs at incA, as the literal accumulator does when no sample index matches"""
    c = lit(8192, 2048, 300, 0.0, 1.0, 1, "--mixed", "--sw-out", "151")
    sw = c["sw"].copy()
    sw[151] = -1
    d, fl, _ = drift(c, path=1, sw=sw)
    inside = (np.abs(c["incA"]) >= MIN_INC) & (np.abs(c["incB"]) >= MIN_INC)
    err = np.abs(d.astype(np.float64) - c["lit"]).max(axis=1)
    print(f"\n[block path: switch at -1] worst error {err[inside].max():.2e} rad, call 151: {err[151]:.2e}")
    assert fl[1] == 1 and np.isfinite(d).all() and inside[151] and err[inside].max() <= TOL


def test_bad_arguments_are_refused(lit):
    c = _base(lit)
    L = g.lib()
    L.dvbt_debug_drift.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    d = np.zeros((300, 64), np.float32)
    fl = np.zeros(4, np.int32)
    ok = [2048, 64, 300, _p(c["sw"]), _p(c["incA"]), _p(c["incB"]), _p(c["entry"]), 0, 0, _p(d), _p(fl), None]
    for i, v in ((0, 4096), (1, 48), (1, 1024), (2, -1), (2, 65537), (3, None), (4, None), (5, None), (6, None), (8, 2), (8, -1), (9, None), (10, None)):
        bad = list(ok)
        bad[i] = v
        assert L.dvbt_debug_drift(*bad) == -1, (i, v)
    assert L.dvbt_debug_drift(*ok) == 0 and tuple(fl) == _applied(c)
