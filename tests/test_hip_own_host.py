"""The owners of gr_dvbt_amd/csrc/hip_own.hpp (device memory, page-locked memory, streams, events) on the CPU.  tests/host/hip_own_host.cpp supplies the HIP
entry points the header uses as counting stubs and runs every owner through scope exit, reset, the moves, refilling, the deque-of-chunks pattern of the streaming
entry and the create functions' pattern with every one of the handle's creations failing in turn.  Built with the address and undefined-behaviour sanitizers and
run as a plain executable: a leak, a double release, a use after release or a release of something never made fails the run or shows in the counts."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_release_everything_once(tmp_path):
    exe = str(tmp_path / "hip_own_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I", os.path.join(ROOT, "gr_dvbt_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "hip_own_host.cpp")])
    out = subprocess.check_output([exe], text=True)
    print(out)
    m = re.search(r"(\d+) allocations, (\d+) live, (\d+) invalid releases, (\d+) errors", out)
    assert m, out
    assert int(m.group(1)) > 0, out
    assert int(m.group(2)) == 0 and int(m.group(3)) == 0 and int(m.group(4)) == 0, out
