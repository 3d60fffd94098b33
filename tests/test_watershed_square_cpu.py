"""The Watershed reward's square (csrc/ssd_ws_square.hpp, shared by host and device) against this machine's libm powf(x, 2):
every float32 in [2^-10, 4096) and a sample of negative and far-out inputs (tests/native/ws_square_check.cpp, plain C++)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_square_equals_libm_powf_exhaustively(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "ws_square_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin",
                           "-I", os.path.join(REPO, "sequential_social_dilemma_games_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "ws_square_check.cpp"), "-o", exe, "-lm"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    n = int(out.split()[-1])
    assert "mismatches 0 " in out and n > 190_000_000, out[-3000:]
