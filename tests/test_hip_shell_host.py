"""hip::core<H, P> of gr_dvbt_amd/host/gr/hip_shell.h -- what every GNU Radio block shell does around its C-ABI call -- on the CPU (tests/host/hip_shell_host.cpp):
stream tags into the dvbt_sideband (known keys translated, unknown ones dropped, rel_offset = offset - nitems_read), the side-band's output tags back at
nitems_written + rel_offset with the right symbol, n_consumed into consume_each, a negative return and a failing create thrown with dvbt_last_error's text,
4096 and 4097 reported output tags against the 4096-entry vector, forecast filling every entry.  The four C-ABI functions are fakes that record and script; gr::block
is the behaving stand-in of oracle/ref_standin/.  Built plain and with the address and undefined-behaviour sanitizers, run as a plain executable: no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitized"])
def test_shell_core_over_fake_abi(tmp_path, flags):
    exe = str(tmp_path / "hip_shell_host")
    subprocess.check_call(["g++", "-std=gnu++11", "-Wall", "-Wno-comment"] + flags +
                          ["-I", os.path.join(ROOT, "oracle", "ref_standin"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gr_dvbt_amd", "host", "gr"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "hip_shell_host.cpp")])
    p = subprocess.run([exe], universal_newlines=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "hip_shell core: 5 works, 0 errors" in p.stdout, p.stdout
