"""CPU checks of the Robust Ensemble (src/graphs/RE.jl): the library's host-only tables (rrrmc_re_tables) against the plain-Python restatement
(tests/re_reference.py) bit for bit, and the restatement against what the reference pins — tracked E == energy(X, C) (RRRMC.jl:250),
check_consistency (DeltaE.jl:120-135), hand-enumerated energies.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import re_reference as RE


@pytest.mark.parametrize("gamma,beta", [(2.0, 0.4), (1.5, 2.0), (0.3, 1.0), (0.05, 7.5)])
def test_re_tables_equal_restatement_bit_for_bit(pkg, gamma, beta):
    for M in range(3, 17):
        dE = np.zeros(M, np.float64)
        e0 = np.zeros(M + 1, np.float64)
        rc = pkg.lib().rrrmc_re_tables(M, gamma, beta, dE, e0)
        assert rc == 0
        rdE, re0 = RE.tables(M, gamma, beta)
        assert dE.tolist() == rdE and e0.tolist() == re0, (M, gamma, beta)
        # fk(-x) = -fk(x) exactly: the classes may be indexed by |mū| (DeltaE.jl:53-60 compares exactly)
        assert (dE == -dE[::-1]).all()
        assert (e0 == e0[::-1]).all()
        # the upper half is allΔE (RE.jl:208-213)
        assert dE[M // 2:].tolist() == RE.all_delta_e(M, gamma, beta)


def test_re_tables_refuse_small_M(pkg):
    dE = np.zeros(8, np.float64)
    e0 = np.zeros(9, np.float64)
    assert pkg.lib().rrrmc_re_tables(2, 1.0, 1.0, dE, e0) == 1
    assert pkg.lib().rrrmc_re_tables(33, 1.0, 1.0, dE, e0) == 3


def test_graph_object_tables_and_checks(pkg):
    X = pkg.Graph0RE(4, 5, 2.0, 0.4)
    assert X.N == 20 and X.model_kind == 11
    dE, e0 = X.tables()
    assert dE.tolist() == RE.tables(5, 2.0, 0.4)[0]
    with pytest.raises(ValueError):
        pkg.Graph0RE(4, 2, 2.0, 0.4)
    with pytest.raises(RuntimeError):
        pkg.REenergies(X)                    # no engine runs it, no configuration given: no stale data


def _brute_energy(Nk, M, gamma, beta, kind, J, s):
    """energy(X, C) from the definitions: Σ_i −log(2cosh(γ μ_i))/β + Σ_k E_slice(k)"""
    E = 0.0
    for i in range(Nk):
        mu = sum(2 * int(s[i * M + k]) - 1 for k in range(M))
        E -= math.log(2 * math.cosh(gamma * mu)) / beta
    for k in range(M):
        sl = [2 * int(s[i * M + k]) - 1 for i in range(Nk)]
        if kind == "skn":
            E += -sum(J[a][b] * sl[a] * sl[b] for a in range(Nk) for b in range(a + 1, Nk))
        elif kind == "sk":
            Jb = [[(int(J[a, b >> 6]) >> (b & 63)) & 1 for b in range(Nk)] for a in range(Nk)]
            E += -sum((2 * Jb[a][b] - 1) * sl[a] * sl[b] for a in range(Nk) for b in range(a + 1, Nk)) / math.sqrt(Nk)
    return E


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_hand_enumerated_energies_nk2_m3(oracle, kind):
    Nk, M, gamma, beta = 2, 3, 1.5, 2.0
    J = None if kind == "empty" else oracle.gen_sk_binary(Nk, 11) if kind == "sk" else oracle.gen_sk_gauss(Nk, 11)
    for bits in itertools.product((0, 1), repeat=Nk * M):
        s = np.array(bits, np.int64)
        X = RE.make_ensemble(Nk, M, gamma, beta, kind, J)
        E = X.energy(s.copy())
        assert abs(E - _brute_energy(Nk, M, gamma, beta, kind, J, s)) < 1e-12
        # delta_energy(X, C, j) = energy after the flip − energy before (RE.jl:312-315), every site
        for j in range(Nk * M):
            t = s.copy()
            t[j] ^= 1
            dE = X.lf0[j] + X.residual(j)
            assert abs(dE - (_brute_energy(Nk, M, gamma, beta, kind, J, t) - E)) < 1e-12


@pytest.mark.parametrize("kind,Nk,M,thr", [("empty", 6, 5, 0.5), ("sk", 10, 8, 0.5), ("skn", 7, 4, 1.0), ("sk", 9, 7, 0.0), ("skn", 5, 3, 0.5)])
def test_restatement_tracks_energy_and_stays_consistent(oracle, kind, Nk, M, thr):
    seed = 977 + Nk * M
    gamma, beta_g, beta = 1.5, 2.0, 1.3
    J = None if kind == "empty" else oracle.gen_sk_binary(Nk, seed) if kind == "sk" else oracle.gen_sk_gauss(Nk, seed)
    X = RE.make_ensemble(Nk, M, gamma, beta_g, kind, J)
    s = RE.config_from_chunks(oracle.init_config(seed, 0, Nk * M), Nk * M)
    run = RE.RrrRun(X, s, beta, seed, oracle, staged_thr=thr, check_E=True)
    run.run(600, 50)
    assert run.accepted > 0
    run.cache.check(s)
    run.check_E = False
    run.run(3000, 100)
    run.cache.check(s)
    assert abs(run.E - RE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s)) < 1e-10
    # standardMC: tracked E after every accepted move
    X2 = RE.make_ensemble(Nk, M, gamma, beta_g, kind, J)
    s2 = RE.config_from_chunks(oracle.init_config(seed, 1, Nk * M), Nk * M)
    E = None
    for part in range(6):
        _, E, acc = RE.standard_mc(X2, s2, beta, 200, 10, seed, oracle, replica=1, it0=200 * part, E=E)
        assert abs(E - RE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s2)) < 1e-10
