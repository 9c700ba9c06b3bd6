"""CPU checks of the replica exchange between contexts: the two symbols, the HIP-free core (rrrmc.jl_amd/csrc/pt_core.hpp with
det_math.hpp's host det_exp) under the host sanitizers against the numpy restatement, the condition the GPU parity cases rely on, the
power of the law test, and ParallelTempering's argument checks."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import boltzmann_law as BL
import exchange_reference as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_in_header_and_table(pkg):
    hdr = open(os.path.join(ROOT, "include", "rrrmc_hip.h")).read()
    for sym in ("rrrmc_exchange_async", "rrrmc_exchange_results"):
        assert re.search(r"RRRMC_API\s+int32_t\s+%s\s*\(" % sym, hdr), sym
        assert sym in pkg.SYMBOLS
    assert hasattr(pkg.Engine, "exchange") and hasattr(pkg.Engine, "exchange_results")
    assert pkg.ParallelTempering is not None


# ---- the core under ASan / UBSan against the restatement ----------------------------------------------------------------------------
def _table_energy(which, r):
    return float((r * 7) % 13 - 6) if which == 0 else float((r * 5) % 11 - 5)


def _cases(oracle):
    """(input line, expected output line) for every case of the table"""
    out = []

    def whole(ba, bb, Ea, Eb, seed, rnd, rep):
        x, u = XR.x_of(ba, bb, Ea, Eb), XR.uniform(oracle, seed, rnd, rep)
        out.append(("A %s %s %s %s %d %d %d" % (float(ba).hex(), float(bb).hex(), float(Ea).hex(), float(Eb).hex(), seed, rnd, rep),
                    "A %s %s %d" % (_c_hex(x), _c_hex(u), XR.accept_x(oracle, x, u))))

    def given(x, u):
        out.append(("X %s %s" % (float(x).hex(), float(u).hex()), "X %d" % XR.accept_x(oracle, x, u)))

    # x = 0 by equal beta and by equal E; x > 0; x < 0 of every size, with big seeds, rounds and replica ids
    whole(0.7, 0.7, -12.0, 5.0, 77, 0, 0)
    whole(0.4, 1.0, -3.5, -3.5, 77, 1, 1)
    whole(1.0, 0.4, -20.0, -4.0, 78, 2, 5)
    whole(0.4, 1.0, 6.0, -4.0, 78, 3, 6)
    for k in range(40):
        whole(0.4 + 0.01 * k, 1.0, -30.0 + 1.7 * k, -2.0 - 0.3 * k, (0xDEADBEEF << 32) | (k * 7919), (1 << 32) + k, (1 << 31) + 13 * k)
        whole(1.0, 0.4 + 0.01 * k, -30.0 + 1.7 * k, -2.0 - 0.3 * k, 5, k, k)
    # x just above and below det_exp's cut at -745.2: above it the result is the smallest subnormal, below it zero
    lo, hi = math.nextafter(-745.2, -math.inf), math.nextafter(-745.2, math.inf)
    for x in (lo, -745.2, hi, -745.0, -746.0, -744.5):
        for u in (0.0, 5e-324, 2.0 ** -53):
            given(x, u)
    whole(1000.0, 0.0, -0.7452, 0.0, 9, 9, 9)                      # x = -745.2 (or its neighbour) from the operands
    whole(0.0, 1000.0, 0.0, -0.7453, 9, 9, 10)
    # u equal to det_exp(x) and one ulp either side
    for x in (-1.0, -0.1, -3.75, -30.0, -700.0, -1e-9):
        e = oracle.det_exp(x)
        for u in (math.nextafter(e, 0.0), e, math.nextafter(e, 1.0)):
            given(x, u)
    given(0.0, 0.999)
    given(math.nan, 0.0)                                             # an energy that is not finite: rejected
    # the mask words and their padding bits
    for R in (1, 31, 32, 33, 63, 64, 65):
        for (ba, bb, seed, rnd) in ((1.0, 0.5, 9, 2), (0.5, 1.0, 11, (1 << 32) + 1)):
            fl = [XR.accept_x(oracle, XR.x_of(ba, bb, _table_energy(0, r), _table_energy(1, r)), XR.uniform(oracle, seed, rnd, r)) for r in range(R)]
            m = XR.mask_words(fl)
            out.append(("M %d %s %s %d %d" % (R, float(ba).hex(), float(bb).hex(), seed, rnd),
                        "M %d %s %d" % (len(m), " ".join("%08x" % w for w in m), sum(fl))))
            assert R % 32 == 0 or int(m[-1]) >> (R % 32) == 0       # the restatement's own padding bits
    return out


def _c_hex(v):
    """a double as C's printf("%a") writes it (glibc): Python's float.hex() pads the mantissa, C does not"""
    if v == 0.0:
        return "-0x0p+0" if math.copysign(1.0, v) < 0 else "0x0p+0"
    h = float(v).hex()                       # [-]0x1.hhhhhhhhhhhhhp[+-]e
    m = re.fullmatch(r"(-?0x[01])\.([0-9a-f]+)p([+-]\d+)", h)
    frac = m.group(2).rstrip("0")
    return "%s%sp%s" % (m.group(1), "." + frac if frac else "", m.group(3))


def test_pt_core_under_asan_and_ubsan_equals_the_restatement(oracle, tmp_path):
    assert shutil.which("g++") is not None, "g++ is needed: this program is the only host check of pt_core.hpp"
    exe = str(tmp_path / "pt_core_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "pt_core_check.cpp"), "-o", exe])
    cases = _cases(oracle)
    tab = tmp_path / "cases.txt"
    tab.write_text("\n".join(c[0] for c in cases) + "\n")
    out = subprocess.run([exe, str(tab)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.strip().split("\n")
    assert got[-1] == "done %d" % len(cases)
    for (inp, want), g in zip(cases, got):
        assert g == want, (inp, g, want)
    # the table holds what it is meant to hold
    verdicts = [w.split()[-1] for (i, w) in cases if i[0] in "AX"]
    assert "0" in verdicts and "1" in verdicts
    assert sum(float.fromhex(w.split()[1]) == 0.0 and w.split()[3] == "1" for (i, w) in cases if i[0] == "A") >= 2          # x = 0 (of either sign) swaps
    sub = [(float.fromhex(i.split()[1]), float.fromhex(i.split()[2]), w) for (i, w) in cases if i[0] == "X"]
    assert any(x < -745.2 and w == "X 0" for x, u, w in sub) and any(-745.2 <= x <= -744.5 and u == 0.0 and w == "X 1" for x, u, w in sub)


# ---- the condition of the GPU parity cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", XR.PARITY_CASES, ids=XR.PARITY_IDS)
def test_parity_cases_last_group_holds_both_verdicts(pkg, oracle, case):
    X = case.make(pkg)
    tail = XR.tail_replicas(case.R)
    Ea = [XR.oracle_energy_after(oracle, X, case.seed_a, case.beta_a, case.iters, r) for r in tail]
    Eb = [XR.oracle_energy_after(oracle, X, case.seed_b, case.beta_b, case.iters, r) for r in tail]
    fl = [XR.accept_x(oracle, XR.x_of(case.beta_a, case.beta_b, a, b), XR.uniform(oracle, case.xseed, case.rnd, r)) for r, a, b in zip(tail, Ea, Eb)]
    print(case.id, tail, fl)
    assert any(fl) and not all(fl), fl


# ---- the law test has room and power -----------------------------------------------------------------------------------------------------
LAW_BETAS = (0.4, 0.7, 1.0)


def law_graph(pkg):
    return pkg.GraphRRG(10, 3, seed=11)


def _law_scores(X, s):
    E = BL.exact_energies(X)
    out = []
    for t, beta in enumerate(LAW_BETAS):
        counts = np.bincount(XR.state_index_pm(s[t]), minlength=len(E))
        out.append(BL.score(counts, BL.boltzmann(E, beta)))
    return out


def test_reference_pt_follows_the_law_and_the_flipped_rule_does_not(pkg):
    X = law_graph(pkg)
    good = _law_scores(X, XR.reference_pt(X.A, X.J, LAW_BETAS, 65536, 100, 4, np.random.default_rng(2025)))
    bad = _law_scores(X, XR.reference_pt(X.A, X.J, LAW_BETAS, 65536, 100, 4, np.random.default_rng(2025), flip_sign=True))
    for beta, g, b in zip(LAW_BETAS, good, bad):
        print("beta %.1f: chi2 %.0f (limit %.0f, %d dof, pooled mass %.4f); flipped rule chi2 %.0f" % (beta, g.chi2, g.limit, g.dof, g.pooled_mass, b.chi2))
        BL.check_pooling(g)
        BL.check_pooling(b)
        assert g.chi2 < g.limit
        assert b.chi2 > b.limit


# ---- ParallelTempering's argument checks (no device: nothing is created before they pass) --------------------------------------------
@pytest.mark.parametrize("betas", [(), (0.5,), (0.5, 0.5), (0.4, 0.7, 0.6), (1.0, 0.7, 0.8), (0.4, math.inf), (math.nan, 0.4), (0.4, -math.inf), "ab", (0.4, None)])
def test_parallel_tempering_refuses_bad_ladders(pkg, betas, monkeypatch):
    made = []
    monkeypatch.setattr(pkg.tempering, "Engine", lambda *a, **k: made.append(1))
    with pytest.raises(ValueError):
        pkg.ParallelTempering(law_graph(pkg), betas, R=4)
    assert not made


def test_parallel_tempering_refuses_bad_R_and_derives_distinct_seeds(pkg, monkeypatch):
    made = []
    monkeypatch.setattr(pkg.tempering, "Engine", lambda *a, **k: made.append(1))
    with pytest.raises(ValueError):
        pkg.ParallelTempering(law_graph(pkg), (0.4, 0.7), R=0)
    assert not made
    seeds = [pkg.ladder_seed(pkg.tempering.DEFAULT_SEED, t) for t in range(64)]
    assert len(set(seeds)) == 64 and pkg.tempering.DEFAULT_SEED not in seeds and all(0 <= s < 2 ** 64 for s in seeds)
    assert (pkg.tempering.check_betas((1.0, 0.7, 0.4)) == np.array([1.0, 0.7, 0.4])).all()
