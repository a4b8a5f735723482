"""All 18 GNU Radio block shells of gr_dvbt_amd/host/gr compiled to objects (not -fsyntax-only) against the BEHAVING stand-in gr::block of oracle/ref_standin/,
the reference's public include/dvbt/*.h (read in place) and include/dvbt_hip.h, then linked into one shared object against gr_dvbt_amd/lib/libdvbt_hip.so with
-Wl,--no-undefined: every dvbt_* entry a shell calls exists in the library with that name, and every GNU Radio name a shell uses is one the stand-in defines.
oracle/Makefile (target `ref`) builds the same objects with the driver into oracle/_ref/libdvbt_shells_hip.so, which tests/test_gpu_gr_shells.py runs."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR = os.path.join(ROOT, "gr_dvbt_amd", "host", "gr")
REF_INC = "/root/reference/include"
LIB = os.path.join(ROOT, "gr_dvbt_amd", "lib")


@pytest.mark.skipif(not os.path.isdir(REF_INC) or shutil.which("g++") is None, reason="needs the reference's public headers (include/dvbt/*.h) and g++")
def test_every_shell_compiles_and_links_against_the_library(tmp_path):
    srcs = sorted(glob.glob(os.path.join(GR, "*_impl.cc")))
    assert len(srcs) == 18
    assert os.path.exists(os.path.join(LIB, "libdvbt_hip.so")), "build() makes gr_dvbt_amd/lib/libdvbt_hip.so"
    inc = ["-I", os.path.join(ROOT, "oracle", "ref_standin"), "-I", REF_INC, "-I", os.path.join(GR, "include"), "-I", os.path.join(ROOT, "include"), "-I", GR]
    jobs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s)[:-3] + ".o"))
        jobs.append((o, subprocess.Popen(["g++", "-std=gnu++11", "-O0", "-fPIC", "-Wall", "-Wno-unused", "-Wno-comment", "-Wno-virtual-move-assign", "-c"] + inc + ["-o", o, s],
                                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for o, p in jobs:
        out = p.communicate()[0].decode()
        assert p.returncode == 0 and "warning" not in out, out[-3000:]
    r = subprocess.run(["g++", "-shared", "-o", str(tmp_path / "libshells.so")] + [o for o, _ in jobs] + ["-Wl,--no-undefined", "-L", LIB, "-ldvbt_hip"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
