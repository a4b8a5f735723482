"""gr_dvbt_amd/csrc/k_drift.hpp on the CPU: the closed form of the reference's float phase accumulator (time potential per increment, binade by binade)
and the parallel fixed point the kernels use for the phase at every call entry, against the literal accumulator (one float addition per sample,
ofdm_sym_acquisition_impl.cc:285-309).  tests/drift/drift_host.cpp includes the header's host-callable arithmetic and replays the kernels' scheme."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("drift") / "drift_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "drift", "drift_host.cpp")])
    return out


def run(exe, N, cp, nsym, eps, jitter, seed=1, *more):
    o = subprocess.check_output([exe, str(N), str(cp), str(nsym), repr(eps), repr(jitter), str(seed), *more], text=True).split()
    return tuple(float(x) for x in o)          # literal wander, residual of the sequential closed form, of the kernels' scheme, entry-phase error of the latter


@pytest.mark.parametrize("N,cp,nsym,eps,jitter", [
    (8192, 256, 1500, 2.3247788, 1e-6),       # +0.37 subcarriers, clean loopback
    (8192, 256, 1500, -1.2566, 1e-6),         # -0.2
    (8192, 256, 1200, 0.1, 1e-7),
    (8192, 256, 1200, 0.0167, 1e-7),          # a small constant offset: the accumulator crawls through the coarse binades
    (8192, 256, 1200, 0.3, 1e-3),             # estimates that jitter (echoes)
    (8192, 256, 1200, -2.32, 0.02),           # ... a lot (noise)
    (2048, 64, 4000, 2.3247788, 1e-6),
    (2048, 64, 3000, 0.05, 1e-4),
    (8192, 1024, 600, 1.0, 1e-4),             # GI 1/8
])
def test_closed_form_reproduces_the_float_accumulator(exe, N, cp, nsym, eps, jitter):
    lit, seq, par, ent = run(exe, N, cp, nsym, eps, jitter)
    assert lit > 5e-5                          # there is something to reproduce
    assert seq < 1e-5 and par < 1e-5           # two orders of magnitude below the wander, well inside the EQ tap's tolerance
    assert ent < 1e-3


@pytest.mark.parametrize("N,cp,nsym,eps,jitter,seed", [
    (8192, 256, 544, 0.02, 3e-3, 1),
    (8192, 256, 3000, 0.01, 1e-3, 1),
    (8192, 256, 600, 0.006, 5e-4, 1),
    (8192, 256, 600, 0.006, 5e-4, 2),
    (2048, 64, 3000, 0.0012, 5e-5, 1),
    (2048, 64, 1100, -0.02, 3e-3, 1),
])
def test_increments_of_a_few_ulps_under_jitter(exe, N, cp, nsym, eps, jitter, seed):
    """the step rint(inc / ulp) * ulp jumps from call to call: three rounds of the fixed point leave 2e-4 .. 1e-3 rad (as much as the wander: 9.7e-4, 9.7e-4, 2.3e-5,
    1.4e-4, 2.4e-4, 2.3e-4 on these rows) and the scheme has to notice and take the recurrence over the calls (k_drift.hpp)"""
    lit, seq, par, ent = run(exe, N, cp, nsym, eps, jitter, seed)
    assert lit > 5e-5
    assert seq < 1e-5 and par < 1e-5
    assert ent < 1e-3


def test_the_oracles_epsilon_on_an_echo_with_a_small_offset(exe):
    """epsilon as the oracle estimates it on 8k QAM64 7/8 behind an echo with a carrier offset of 0.003 subcarriers (tests/golden/make_drift_golden.py):
    0.0087 .. 0.0331, increments of 4 .. 17 ulp of the accumulator's coarsest binade"""
    lit, seq, par, ent = run(exe, 8192, 256, 544, 0.0, 0.0, 1, "--eps-file", os.path.join(ROOT, "tests", "golden", "drift_eps_8k_echo_cfo.txt"))
    assert lit > 5e-5
    assert seq < 1e-5 and par < 1e-5
    assert ent < 1e-3


@pytest.mark.parametrize("eps,jitter", [(2.3247788, 1e-6), (-2.32, 0.02)])
def test_a_segment_of_the_benchmarks_length(exe, eps, jitter):
    """17,680 calls of 8k, the benchmark's segment.  The entry phase is printed, not bounded: over 1.5e8 steps the closed form's entry phase drifts from the
    literal accumulator's by 8e-4 .. 1.6e-2 rad (every binade crossing contributes a fraction of a step), which is one common rotation of a whole symbol --
    the equaliser divides it out -- and moves the deviations INSIDE the call only through where the binade crossings fall: the residuals below hold."""
    lit, seq, par, ent = run(exe, 8192, 256, 17680, eps, jitter)
    print(f"\n[17,680 calls, eps {eps}, jitter {jitter}] wander {lit:.2e}, sequential {seq:.2e}, kernels' scheme {par:.2e}, entry phase {ent:.2e} rad")
    assert lit > 5e-5
    assert seq < 1e-5 and par < 1e-5


def test_a_limit_of_the_closed_form_itself(exe):
    """17,680 calls of 8k at epsilon 0.0167 with a jitter of 1e-7: the increment stays beside a rounding tie of one binade for the whole segment and the closed
    form itself (the sequential recurrence: no fixed point involved) is 3.3e-5 rad away from the literal accumulator.  Held only to 1.35e-4 rad, what the
    tolerance of the equalised-carrier tap corresponds to (1e-3 of the spacing; 5e-4 rad are 3.7e-3 of it, k_drift.hpp)."""
    lit, seq, par, ent = run(exe, 8192, 256, 17680, 0.0167, 1e-7)
    print(f"\n[17,680 calls, eps 0.0167, jitter 1e-7] wander {lit:.2e}, sequential {seq:.2e}, kernels' scheme {par:.2e}, entry phase {ent:.2e} rad")
    assert lit > 5e-5
    assert seq < 1.35e-4 and par < 1.35e-4
