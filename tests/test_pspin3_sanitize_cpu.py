"""The HIP-free 3-spin code (rrrmc.jl_amd/csrc/pspin_core.hpp and the first part of host_pspin.hpp: the partner table, delta_energy and
energy over it, the generator, the validation and its refusals) compiled with g++ -fsanitize=address,undefined into the stand-alone
tests/pspin_core_check.cpp and run: every index of generated tables — the limits N = 65 535 and K = 16 included — stays in bounds, and
pspin_delta / pspin_energy equal the direct sum over the triples at bit offsets 0, 1, 31 and 33.  A program of its own: nothing loaded
into Python and nothing on the GPU is sanitized."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pspin_core_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pspin_core_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "pspin_core_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all invariants hold" in out.stdout
