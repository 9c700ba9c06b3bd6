"""The Topological Local Entropy ensemble against the exact Boltzmann law: 8 spins, 256 states enumerated, with the statistic, thresholds and
runner of tests/boltzmann_law.py unchanged.  The energies are written here from the definition (TLE.jl:79-142, 413-435) — not taken from the
library nor from tests/tle_reference.py:
    E = -γT Σ_i σc_i μ_i - (λT / 2) Σ_i Σ_{i2 ∈ ∂i} σc_i σc_i2 Σ_k σ_(i,k) σ_(i2,k) + Σ_k E_slice(replica k),
μ_i = Σ_k σ_(i,k), the centre's own slice energy left out.  Nk = 2 keeps the bins the exact law pools within the runner's caps."""
import numpy as np
import pytest

import boltzmann_law as BL

pytestmark = pytest.mark.gpu

GAMMA, LAMBDA, BETA_G, BETA = 0.6, 0.4, 1.2, 0.8
SAT_A, SAT_J = [[0, 1], [0, 1], [1]], [[1, 0], [0, 0], [1]]          # x0 ∨ ¬x1, ¬x0 ∨ ¬x1, x1


def _violated(A, J):
    """s [S, N] of ±1 -> the number of clauses none of whose literals holds (SAT.jl:117-123), as Float64"""
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


def energy_tle(slice_energy, Nk, M, neighb, gamma, lam, beta_g, sg):
    gT, lT = gamma / beta_g, lam / beta_g
    s = sg.reshape(-1, Nk, M + 1)                                   # site j = spin j // (M+1), row j % (M+1); row 0 the centre
    c, rep = s[:, :, 0], s[:, :, 1:]
    E = -gT * (c * rep.sum(axis=2)).sum(axis=1)
    top = np.zeros(len(s))
    for i, ni in enumerate(neighb):
        for i2 in ni:
            top += c[:, i] * c[:, i2] * (rep[:, i, :] * rep[:, i2, :]).sum(axis=1)
    E = E - lT * top / 2
    if slice_energy is not None:
        for k in range(M):
            E = E + slice_energy(rep[:, :, k])
    return E


def _sk(pkg):
    return pkg.GraphSKTLE(2, 3, GAMMA, LAMBDA, BETA_G, seed=21)


def _sat(pkg):
    return pkg.GraphSATTLE(pkg.GraphSAT.from_clauses(2, SAT_A, SAT_J), 3, GAMMA, LAMBDA, BETA_G)


def exact(pkg, which):
    X = _sk(pkg) if which == "sk" else _sat(pkg)
    sg = 2 * BL.enumerate_states(X.N) - 1
    sl = (lambda s: BL.energy_sk_binary(X.J, 2, s)) if which == "sk" else _violated(SAT_A, SAT_J)
    return X, energy_tle(sl, 2, 3, [[1], [0]], GAMMA, LAMBDA, BETA_G, sg)


@pytest.mark.parametrize("which", ["sk", "sat"])
@pytest.mark.parametrize("sampler,iters,seed", [("std", 2700, 191), ("rrr", 1350, 192)])
def test_tle_follows_the_boltzmann_law(pkg, which, sampler, iters, seed):
    case = BL._case("%s-GraphTLE-%s-2-3-tle_kernels" % (sampler, which), None, sampler, BETA, iters, seed)
    X, E = exact(pkg, which)
    assert X.N == 8 and X.Nk == 2 and X.M == 3 and X.neighb == [[1], [0]] and len(E) == 256
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))
