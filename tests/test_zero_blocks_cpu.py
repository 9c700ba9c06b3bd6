"""The host helper that tells a launch which leading blocks of its thresholds are all zero (rrrmc.jl_amd/csrc/host_plan.hpp:
zero_blocks / zero_pattern; the sweep kernel's specialised builds are selected by it) against a recomputation in exact integer
arithmetic, for the beta list of tests/test_gpu_sweep_zero_blocks.py at K = 1 .. 7.  The HIP-free host code is compiled with g++ into a
stand-alone program (tests/zero_blocks_check.cpp), as tests/test_sanitizers.py does with tests/host_sanitize.cpp — here with the
sanitizers on as well."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = [0.3, 0.5, 1.0, 1.5, 3.0, 6.0, 0.0, 2.0, 50.0]
NBLOCKS = 3


def _zb(beta, K):
    out = []
    for n in range((K + 1) // 2):
        p = math.exp(-beta * 2.0 * (K - 2 * n))
        if p >= 1.0:                                   # always accepted: counts as generic
            out.append(0)
            continue
        T = math.ceil(Fraction(p) * 2 ** 64)            # ceil(p 2^64), exact: Fraction(p) is the double's value
        b = 0
        while b < NBLOCKS and (T >> (60 - 4 * b)) & 0xF == 0:
            b += 1
        out.append(b)
    return out


def test_zero_blocks_equal_an_exact_recomputation(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "zero_blocks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "zero_blocks_check.cpp"), "-o", exe])
    out = subprocess.run([exe] + [repr(b) for b in BETAS], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    assert len(lines) == 7 * len(BETAS)
    seen = {}
    for f in lines:
        beta, K, pat, zb = float(f[0]), int(f[1]), int(f[2]), [int(x) for x in f[3:]]
        want = _zb(beta, K)
        assert zb == want, (beta, K)
        assert pat == sum(z << (2 * n) for n, z in enumerate(want)), (beta, K)
        assert all(a >= b for a, b in zip(zb, zb[1:])), (beta, K)       # T_0 <= T_1 <= ...: the colder class has at least as many
        seen[(beta, K)] = tuple(zb)
    # the patterns the GPU parity file is built around
    assert [seen[(b, 3)] for b in (0.3, 0.5, 1.0, 1.5, 3.0, 6.0)] == [(0, 0), (1, 0), (2, 0), (3, 1), (3, 2), (3, 3)]
    assert seen[(1.0, 6)] == (3, 2, 1) and seen[(1.0, 7)] == (3, 3, 2, 0)
    assert seen[(0.0, 3)] == (0, 0) and seen[(50.0, 3)] == (3, 3)
