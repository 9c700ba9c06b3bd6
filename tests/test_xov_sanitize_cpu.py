"""The HIP-free planning core of the cross-replica overlaps (rrrmc.jl_amd/csrc/xov_core.hpp: tile grid, same-slot triangle, batches of
slot pairs and their distinct-slot lists, caps, histogram form) compiled with g++ -fsanitize=address,undefined into the stand-alone
tests/xov_core_check.cpp and run.  A program of its own: nothing loaded into Python and nothing on the GPU is sanitized."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_xov_core_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "xov_core_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "xov_core_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all invariants hold" in out.stdout
