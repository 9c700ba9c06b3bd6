"""The ensembles over sparse Float64 slices against the exact Boltzmann law on enumerable systems: EA(L=2, D=2) — Nk = 4, every bond doubled —
with GraphEARE M = 3 (N = 12, 4096 states) and GraphEALE / GraphEATLE M = 3 (N = 16, 65 536 states), with the statistic, thresholds, R and
power of tests/boltzmann_law.py unchanged.  The energies are written from the reference's formulas — the slices by
boltzmann_law.energy_sparse_f64 (EA.jl:584-611), the Robust Ensemble by boltzmann_law.energy_re (RE.jl:265-281), the two Local Entropy
ensembles by the definition tests/test_gpu_tle_boltzmann.py states (LE.jl:242-258 is its λ = 0 case) — not taken from the library nor from
tests/sparse_slice_reference.py.

The sampler's β of each case comes from the exact law alone: with 65 536 chains the states whose expected count is below 5 are pooled, and
the runner asks that they hold at most 5 % of the mass (check_pooling, which this test runs: a β that is too low fails there, whatever the
sampler does).  Each β is at, or a little above, the lowest that this rule allows on the instance, because relaxation slows exponentially in β; the run
lengths are burn-in, not a bound (profiles/r18/sparse_ens.md has the figures they were chosen by)."""
import pytest

import boltzmann_law as BL
from test_gpu_tle_boltzmann import energy_tle

pytestmark = pytest.mark.gpu

GAMMA, LAMBDA, BETA_G, SEED_J = 0.6, 0.4, 1.2, 21
BETA = {"re": 1.0, "le": 1.5, "tle": 1.2}


def _graph(pkg, fam):
    if fam == "re":
        return pkg.GraphEARE(2, 2, 3, GAMMA, BETA_G, seed=SEED_J)
    if fam == "le":
        return pkg.GraphEALE(2, 2, 3, GAMMA, BETA_G, seed=SEED_J)
    return pkg.GraphEATLE(2, 2, 3, GAMMA, LAMBDA, BETA_G, seed=SEED_J)


def exact(pkg, fam):
    X = _graph(pkg, fam)
    A, J = X.X1.A, X.X1.J
    sg = 2 * BL.enumerate_states(X.N) - 1
    sl = lambda s: BL.energy_sparse_f64(A, J, s)
    if fam == "re":
        return X, BL.energy_re(sl, 4, 3, GAMMA, BETA_G, sg)
    neighb = [sorted(set(row.tolist())) for row in A]          # neighbors(g0, i) = uA[i]: each lattice neighbour once
    assert all(len(ni) == 2 for ni in neighb)
    return X, energy_tle(sl, 4, 3, neighb, GAMMA, LAMBDA if fam == "tle" else 0.0, BETA_G, sg)


@pytest.mark.parametrize("fam", ["re", "le", "tle"])
@pytest.mark.parametrize("sampler,iters,seed", [("std", 120000, 291), ("rrr", 40000, 292)])
def test_sparse_ensembles_follow_the_boltzmann_law(pkg, fam, sampler, iters, seed):
    case = BL._case("%s-GraphEA%s-2-2-3" % (sampler, fam.upper()), None, sampler, BETA[fam], iters, seed)
    X, E = exact(pkg, fam)
    assert X.Nk == 4 and X.M == 3 and X.K == 4 and len(E) == 1 << X.N and X.N == (12 if fam == "re" else 16)
    if fam == "tle":
        assert X.neighb == [[1, 2], [0, 3], [0, 3], [1, 2]]
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))
