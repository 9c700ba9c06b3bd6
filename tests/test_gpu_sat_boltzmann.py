"""Random K-SAT against the exact Boltzmann law: 9 spins, 512 states enumerated, with the statistic, thresholds and runner of
tests/boltzmann_law.py unchanged.  The energies are written here from the definition — the number of clauses without a true literal
(SAT.jl:117-123) — not taken from the library."""
import numpy as np
import pytest

import boltzmann_law as BL

pytestmark = pytest.mark.gpu


def _violated(A, J):
    """s [S, N] of ±1 -> the number of clauses none of whose literals holds, as Float64 (the engine reports SAT energies so)"""
    def f(s):
        up = s > 0
        E = np.zeros(len(s), np.float64)
        for Aa, Ja in zip(A, J):
            sat = np.zeros(len(s), bool)
            for i, j in zip(Aa, Ja):
                sat |= up[:, i] == bool(j)
            E += ~sat
        return E
    return f


def _sat9(pkg):
    return pkg.GraphSAT(9, 3, 20 / 9, seed=1)                      # N = 9, 20 three-literal clauses


def _satre(pkg):
    return pkg.GraphSATRE(3, 2, 4 / 3, 3, 0.6, 1.2, seed=2)        # Nk = 3, 4 two-literal clauses, M = 3: 9 sites


@pytest.mark.parametrize("build,env", [("sat_wave_kernel", {"RRRMC_SAT_WAVE": "1"}), ("sat_standard_kernel", {"RRRMC_SAT_NO_WAVE": "1"})])
def test_graph_sat_follows_the_boltzmann_law(pkg, build, env):
    case = BL._case("std-GraphSAT-9-20-%s" % build, _sat9, "std", 1.0, 2700, 181, env=env)
    X = _sat9(pkg)
    assert X.N == 9 and X.M == 20 and X.K == 3
    sg = 2 * BL.enumerate_states(X.N) - 1
    E = _violated(X.A, X.J)(sg)
    assert len(np.unique(E)) >= 5                                  # at least 5 populated energy levels
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))


@pytest.mark.parametrize("sampler,iters,seed", [("std", 2700, 182), ("rrr", 1350, 183)])
def test_graph_sat_re_follows_the_boltzmann_law(pkg, sampler, iters, seed):
    case = BL._case("%s-GraphSATRE-3-3-re_kernels" % sampler, _satre, sampler, 0.8, iters, seed)
    X = _satre(pkg)
    assert X.N == 9 and X.Nk == 3 and X.M == 3 and X.X1.M == 4
    sg = 2 * BL.enumerate_states(X.N) - 1
    E = BL.energy_re(_violated(X.X1.A, X.X1.J), X.Nk, X.M, X.gamma, X.beta, sg)
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))
