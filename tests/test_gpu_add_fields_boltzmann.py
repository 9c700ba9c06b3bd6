"""GraphAddFields / GraphAddSubFields against the exact Boltzmann law: 9 spins over a GraphSAT, 512 states enumerated, with the statistic,
thresholds and runner of tests/boltzmann_law.py unchanged and the iterations and β of the CPU twin (tests/test_add_fields_cpu.py).
GraphAddSubFields follows exp(-β E_g) whatever the fields; GraphAddFields follows exp(-β (Σ h σ + E_g)).  The energies are written
here from the definitions, not taken from the library."""
import numpy as np
import pytest

import boltzmann_law as BL
from test_add_fields_cpu import BL_BETA, BL_ITERS, bl_instance, violated

pytestmark = pytest.mark.gpu


def _graph(pkg, sub):
    g = pkg.GraphSAT(9, 3, 20 / 9, seed=1)                         # N = 9, 20 three-literal clauses
    return (pkg.GraphAddSubFields if sub else pkg.GraphAddFields)(bl_instance(), g)


@pytest.mark.parametrize("sampler,env,seed", [("rrr", {}, 191), ("rrr", {"RRRMC_AF_NO_LDS": "1"}, 192), ("std", {}, 193)], ids=["rrr-lds", "rrr-global", "std"])
@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
def test_the_wrappers_follow_the_boltzmann_law(pkg, sub, sampler, env, seed):
    iters = BL_ITERS if sampler == "rrr" else 2700                 # standardMC: the iterations of the stand-alone GraphSAT's row
    case = BL._case("%s-%s-9-af_kernels" % (sampler, "GraphAddSubFields" if sub else "GraphAddFields"), None, sampler, BL_BETA, iters, seed + 10 * sub, env=env)
    X = _graph(pkg, sub)
    assert X.N == 9 and X.X1.M == 20
    sg = 2 * BL.enumerate_states(X.N) - 1
    E = violated(X.X1.A, X.X1.J, sg) + (0.0 if sub else sg @ X.fields)
    assert len(np.unique(violated(X.X1.A, X.X1.J, sg))) >= 5
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))
