"""CPU checks of the cross-replica overlaps: the numpy reference the GPU tests compare against equals the oracle's pm1dot, the
histogram's counting rule, overlap_moments against direct summation, and the two new symbols in the header and the Python table."""
import math
import os
import re

import numpy as np
import pytest

import xov_reference as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    """dict equality with NaN == NaN and floats compared bit for bit"""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], float) and math.isnan(a[k]):
            assert isinstance(b[k], float) and math.isnan(b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("N", [10, 64, 65, 130])
def test_reference_matrix_and_hist_match_pm1dot(pkg, oracle, N):
    rng = np.random.default_rng(4000 + N)
    RA, RB = 7, 5
    bitsA = rng.integers(0, 2, (RA, N), dtype=np.uint8)
    bitsB = rng.integers(0, 2, (RB, N), dtype=np.uint8)
    bitsB[1] = bitsA[2]                                    # one identical pair: q = N
    bitsB[3] = 1 - bitsA[0]                                # one opposite pair: q = -N
    cA, cB = pkg.Config.from_bits(bitsA).s, pkg.Config.from_bits(bitsB).s
    q = XR.cross_matrix(bitsA, bitsB, N)
    assert q.shape == (RA, RB) and q[2, 1] == N and q[0, 3] == -N
    for i in range(RA):
        for j in range(RB):
            assert q[i, j] == oracle.pm1dot(cA[i], cB[j], N)
            assert q[i, j] == XR.pm1dot_cols(bitsA[i], bitsB[j], N)
    # the counting rule: r1 < r2 within one slot, every r1 != r2 between two slots
    hs = XR.hist([(bitsA, bitsA, True)], N)
    hd = XR.hist([(bitsA, bitsA[::-1].copy(), False)], N)
    assert hs.sum() == RA * (RA - 1) // 2 and hd.sum() == RA * (RA - 1)
    want = np.zeros(N + 1, np.int64)
    for i in range(RA):
        for j in range(i + 1, RA):
            want[(N - oracle.pm1dot(cA[i], cA[j], N)) // 2] += 1
    assert (hs == want).all()
    assert (XR.hist([(bitsA, bitsA, True), (bitsA, bitsA[::-1].copy(), False)], N) == hs + hd).all()


@pytest.mark.parametrize("N", [10, 65, 131])
def test_overlap_moments_equal_direct_summation(pkg, N):
    rng = np.random.default_rng(5000 + N)
    R = 9
    bits = rng.integers(0, 2, (R, N), dtype=np.uint8)
    q = XR.cross_matrix(bits, bits, N)
    qs = [q[i, j] for i in range(R) for j in range(i + 1, R)]
    m = pkg.overlap_moments(XR.hist([(bits, bits, True)], N), N)
    _same(m, XR.moments(qs, N))
    assert m["pairs"] == R * (R - 1) // 2 and 0.0 < m["q2"] <= 1.0 and m["q4"] <= m["q2"]


def test_overlap_moments_edge_cases(pkg):
    N, R = 33, 6
    bits = np.tile(np.random.default_rng(1).integers(0, 2, (1, N), dtype=np.uint8), (R, 1))      # all replicas equal: q = N everywhere
    h = XR.hist([(bits, bits, True)], N)
    assert h[0] == R * (R - 1) // 2 and h[1:].sum() == 0
    m = pkg.overlap_moments(h, N)
    _same(m, {"pairs": R * (R - 1) // 2, "q2": 1.0, "q4": 1.0, "binder": 1.0, "absq": 1.0})
    _same(m, XR.moments([N] * (R * (R - 1) // 2), N))
    empty = pkg.overlap_moments(np.zeros(N + 1, np.int64), N)
    assert empty["pairs"] == 0 and all(math.isnan(empty[k]) for k in ("q2", "q4", "binder", "absq"))
    _same(empty, XR.moments([], N))
    # N even, every pair at q = 0: <q^2> = 0 and no Binder ratio
    z = np.zeros(11, np.int64)
    z[5] = 4
    mz = pkg.overlap_moments(z, 10)
    assert mz["pairs"] == 4 and mz["q2"] == 0.0 and mz["q4"] == 0.0 and mz["absq"] == 0.0 and math.isnan(mz["binder"])
    # counts beyond 2^53 stay exact: the sums are Python integers
    big = np.zeros(4, np.int64)
    big[0], big[1] = 2 ** 60, 2 ** 60
    mb = pkg.overlap_moments(big, 3)
    assert mb["pairs"] == 2 ** 61 and mb["q2"] == (9 + 1) / (2 * 9) and mb["q4"] == (81 + 1) / (2 * 81)
    with pytest.raises(ValueError):
        pkg.overlap_moments(np.zeros(5, np.int64), 10)


def test_header_and_python_table_have_both_symbols(pkg):
    hdr = open(os.path.join(ROOT, "include", "rrrmc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"RRRMC_API\s+int32_t\s+rrrmc_cross_overlaps\s*\(([^)]*)\)\s*;", hdr)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["ctx", "npairs", "slotA", "slotB", "a0", "nA", "b0", "nB", "q_out"]
    m = re.search(r"RRRMC_API\s+int32_t\s+rrrmc_overlap_hist\s*\(([^)]*)\)\s*;", hdr)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["ctx", "npairs", "slotA", "slotB", "hist_out"]
    assert "rrrmc_cross_overlaps" in pkg.SYMBOLS and "rrrmc_overlap_hist" in pkg.SYMBOLS
    assert callable(pkg.parsexovs) and callable(pkg.overlap_moments)
    assert hasattr(pkg.Engine, "cross_overlaps") and hasattr(pkg.Engine, "overlap_hist")
