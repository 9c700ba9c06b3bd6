"""The CPU oracle under the exact Boltzmann law: the case table of tests/boltzmann_law.py through the oracle's entry points, with fewer chains
(`cpu_R`).  Same energies from the definition, same χ² limit, same pooling conditions, same power check as tests/test_gpu_boltzmann.py; a row
whose reduced run cannot tell 1.1 β apart names the factor it can (`cpu_power`).  The Robust Ensemble rows have no entry point in the oracle
(tests/re_reference.py is plain Python: thousands of chains are out of its reach) and run on the device only."""
import pytest

import boltzmann_law as BL

CPU_CASES = [c for c in BL.CASES if c.cpu_R is not None]
_E = {}


@pytest.mark.parametrize("case", CPU_CASES, ids=[c.id for c in CPU_CASES])
def test_oracle_chains_follow_the_boltzmann_law(pkg, oracle, case):
    X = case.model(pkg)
    if case.model not in _E:
        _E[case.model] = BL.exact_energies(X)
    E = _E[case.model]
    idx, Etr, Es_last = BL.run_oracle(oracle, case, X, case.cpu_R)
    v = BL.judge(case, E, idx, Es_last, power=case.cpu_power)
    print("%s: chi2 %.1f (limit %.1f, %d dof, smallest expected %.1f, pooled mass %.4f); at %.1f beta %.1f (limit %.1f)"
          % (case.id, v.law.chi2, v.law.limit, v.law.dof, v.law.min_expected, v.law.pooled_mass, case.cpu_power, v.power.chi2, v.power.limit))
    if Etr is not None:
        BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(v)


def test_every_energy_function_is_invariant_under_the_global_flip(pkg):
    """none of these models has a field: E(σ) = E(−σ) (for the ensembles: of all slices at once) — a cheap check of the enumeration order and
    of the site layouts (slice-major GraphQuant, replica-minor GraphRobustEnsemble) that the energy functions assume"""
    seen = set()
    for case in BL.CASES:
        if case.model in seen:
            continue
        seen.add(case.model)
        E = BL.exact_energies(case.model(pkg))
        assert len(E) == 2 ** case.model(pkg).N and (abs(E - E[::-1]) <= 1e-12).all(), case.id


def test_the_statistic_pools_and_has_power():
    import numpy as np
    p = np.array([0.5, 0.3, 0.1999, 0.00005, 0.00005])
    sc = BL.score(np.array([5000, 3000, 1999, 1, 0]), p)
    assert sc.dof == 3 and abs(sc.pooled_expected - 1.0) < 1e-9 and abs(sc.pooled_mass - 1e-4) < 1e-12 and sc.chi2 < 1e-6
    with pytest.raises(AssertionError):
        BL.check_pooling(sc)                                           # the pooled bin's own expected count is 1 < 5
    # a 10 % error in β on a two-level system: 2^16 draws from the law at β = 1 fail the law at 1.1 β and pass their own
    E = np.array([0.0] * 8 + [2.0] * 8)
    counts = np.round(65536 * BL.boltzmann(E, 1.0))
    own, wrong = BL.score(counts, BL.boltzmann(E, 1.0)), BL.score(counts, BL.boltzmann(E, 1.1))
    assert own.chi2 < 1e-2 and wrong.chi2 > wrong.limit and own.dof == 15
