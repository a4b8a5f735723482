"""The GNU Radio block shells of the transmit blocks (gr_dvbt_amd/host/gr): one per block of the TX chain, deriving from the reference's own public class
(convolutional_interleaver from gr::sync_interpolator).  As tests/test_gr_shells.py: a syntax check only, g++ -fsyntax-only against the reference's
include/dvbt/*.h (read in place, never copied) and the declarations of tests/gr_syntax/; it builds and runs nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR = os.path.join(ROOT, "gr_dvbt_amd", "host", "gr")
REF_INC = "/root/reference/include"

BLOCKS = ["energy_dispersal", "reed_solomon_enc", "convolutional_interleaver", "inner_coder", "bit_inner_interleaver", "dvbt_map", "reference_signals"]


def test_every_transmit_block_has_a_shell_in_the_build():
    for b in BLOCKS:
        assert os.path.exists(os.path.join(GR, b + "_impl.h")) and os.path.exists(os.path.join(GR, b + "_impl.cc")), b
    cm = open(os.path.join(GR, "CMakeLists.txt")).read()
    assert all(b + "_impl.cc" in cm for b in BLOCKS)


@pytest.mark.skipif(not os.path.isdir(REF_INC) or shutil.which("g++") is None, reason="needs the reference's public headers and g++")
@pytest.mark.parametrize("block", BLOCKS)
def test_transmit_shell_matches_the_reference_interface(block):
    cmd = ["g++", "-std=gnu++11", "-fsyntax-only", "-Wall", "-Wno-unused", "-Wno-comment", "-I", os.path.join(ROOT, "tests", "gr_syntax"), "-I", REF_INC,
           "-I", os.path.join(GR, "include"), "-I", os.path.join(ROOT, "include"), "-I", GR, os.path.join(GR, block + "_impl.cc")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
