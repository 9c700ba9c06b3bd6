"""The HIP-free Topological Local Entropy code (rrrmc.jl_amd/csrc/tle_core.hpp: the topology checks, the neighbour program, the level and
class-code tables) compiled with g++ -fsanitize=address,undefined into the stand-alone tests/tle_core_check.cpp and run.  A program of its
own: nothing loaded into Python and nothing on the GPU is sanitized."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tle_core_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "tle_core_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "tle_core_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all invariants hold" in out.stdout
