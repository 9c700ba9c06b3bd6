"""GraphMixed against the exact Boltzmann law: 9 spins, GraphMixed(GraphSK(9), GraphEANormal(3, 2), GraphSAT(9, 3, 2.0)), 512 states
enumerated, 65 536 chains, with the statistic, thresholds and runner of tests/boltzmann_law.py unchanged: standardMC in both builds, and
rrrMC through GraphAddSubFields (whose stationary law is the mix's own, whatever the fields).  The energies are written here from the
definitions, not taken from the library.

β = 0.6.  From the exact law of this seeded instance alone (no device; profiles/r19/mixed.md): the states whose expected count is below 5
hold 0.54 % of the mass and expect 357 chains together; at 1.1 β they hold 0.48 % and expect 317, and the expected χ² of the law's own
counts against the law at 1.1 β is 1870 for a limit of 247 (7.6 times)."""
import numpy as np
import pytest

import boltzmann_law as BL
from test_add_fields_cpu import violated

pytestmark = pytest.mark.gpu

BETA = 0.6
STD_ITERS, RRR_ITERS = 2700, 1000


def instance(pkg):
    sk, ea, sat = pkg.GraphSK(9), pkg.GraphEANormal(3, 2), pkg.GraphSAT(9, 3, 2.0)
    sg = 2 * BL.enumerate_states(9) - 1
    E = BL.energy_sk_binary(sk.J, 9, sg) + BL.energy_sparse_f64(ea.A, ea.J, sg) + violated(sat.A, sat.J, sg)
    return pkg.GraphMixed(sk, ea, sat), E


@pytest.mark.parametrize("sampler,env,seed", [("std", {"RRRMC_MIXED_NO_WAVE": "1"}, 291), ("std", {"RRRMC_MIXED_WAVE": "1"}, 292), ("rrr", {}, 293)],
                         ids=["std-thread", "std-wave", "rrr-AddSubFields"])
def test_the_mix_follows_the_boltzmann_law(pkg, sampler, env, seed):
    X, E = instance(pkg)
    assert X.N == 9 and len(np.unique(np.round(E, 9))) > 400
    if sampler == "rrr":
        X = pkg.GraphAddSubFields(np.array([0.5, -0.5, 0.0, 1.0, -1.0, 0.5, 0.0, -0.5, 1.0]), X)
    case = BL._case("%s-GraphMixed-9" % sampler, None, sampler, BETA, STD_ITERS if sampler == "std" else RRR_ITERS, seed, env=env)
    assert case.R == 65536 and case.observable == "state"
    with BL.with_env(env):
        idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    v = BL.judge(case, E, idx, Es_last)
    print("chi2 %s: law %.1f (limit %.1f, %d dof), at 1.1 beta %.1f (limit %.1f)" % (case.id, v.law.chi2, v.law.limit, v.law.dof, v.power.chi2, v.power.limit))
    BL.assert_verdict(v)
