"""Every sampler x model family of the HIP library against the exact Boltzmann law (tests/boltzmann_law.py): many independent chains on a
system small enough to enumerate, their final configurations (or last sampled energies) scored against exp(-βE)/Z with energies written from
the reference's definitions — not against the CPU oracle, which shares the library's author and reading.  Every row also asserts the pooling
conditions of the χ² test, that the same counts FAIL the law at 1.1 β, and that the energy each chain tracked is the definition's energy of
its final state.  profiles/r10/boltzmann.md lists what the oracle predicted for every row and what the device gave."""
import pytest

import boltzmann_law as BL

pytestmark = pytest.mark.gpu

_E = {}


def _energies(case, X):
    key = case.model                                   # rows that share an instance share its enumeration
    if key not in _E:
        _E[key] = BL.exact_energies(X)
    return _E[key]


@pytest.mark.parametrize("case", BL.CASES, ids=BL.CASE_IDS)
def test_chains_follow_the_boltzmann_law(pkg, case):
    X = case.model(pkg)
    assert X.N <= 10
    E = _energies(case, X)
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    v = BL.judge(case, E, idx, Es_last)
    print("%s: chi2 %.1f (limit %.1f, %d dof, smallest expected %.1f, pooled mass %.4f); at 1.1 beta %.1f (limit %.1f)"
          % (case.id, v.law.chi2, v.law.limit, v.law.dof, v.law.min_expected, v.law.pooled_mass, v.power.chi2, v.power.limit))
    BL.assert_tracked_energy(E, idx, Etr)
    if case.observable == "energy":                    # bklMC / wtmMC stop at their last sample: it is the tracked energy
        BL.assert_tracked_energy(E, idx, Es_last)
    BL.assert_verdict(v)
