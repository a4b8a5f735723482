"""The index arithmetic that every user of the LDS FFT (gr_dvbt_amd/csrc/k_fft.hpp) relies on, on the CPU: where bin k stands after fft_dif_lds (fft_pos_of_bin
against the digit reversal over the pass radices, restated in tests/host/fft_index_host.cpp), the padding of the LDS image (fpad) and the size of the workspace
(fft_lds_bytes), for every size of the dvbt_fft block.  A plain C++ compiler takes the header's host part (its device part is for a HIP compiler alone); built with
the address and undefined-behaviour sanitizers and run as a plain executable: no HIP runtime call, no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fft_index_arithmetic(tmp_path):
    exe = str(tmp_path / "fft_index_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I", os.path.join(ROOT, "gr_dvbt_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "fft_index_host.cpp")])
    p = subprocess.run([exe], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    per_size = re.findall(r"^N (\d+): radices ([\d ]+), (\d+) bytes, (\d+) errors$", p.stdout, re.M)
    assert [int(m[0]) for m in per_size] == [64, 128, 256, 512, 1024, 2048, 4096, 8192], p.stdout
    assert all(int(m[3]) == 0 for m in per_size), p.stdout
    radices = {int(m[0]): m[1] for m in per_size}
    assert radices[2048] == "16 16 4 2" and radices[8192] == "16 16 16 2", p.stdout
    assert re.search(r"^8 sizes, 0 errors$", p.stdout, re.M), p.stdout
