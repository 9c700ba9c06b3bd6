"""GraphPercXEntr against the exact Boltzmann law: N = 5 synapses, P = 3 patterns, 32 states enumerated, with the statistic, thresholds and
runner of tests/boltzmann_law.py unchanged and the β, iterations and seeds of the CPU twin (tests/test_perc_xentr_cpu.py, where the
restatement alone passes the same verdict and the choice of β and iterations is written down).  standardMC stand-alone in both kernel
builds, and rrrMC on GraphAddSubFields over it, which follows exp(-β E_g) whatever the fields.  The energies are written from the
definition (log1p ∘ exp of the overlaps, no table), not taken from the library."""
import numpy as np
import pytest

import boltzmann_law as BL
from test_perc_xentr_cpu import BL_BETA, BL_ITERS, BL_SEEDS, bl_energies, bl_fields, bl_graph

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which,env,build", [("std-thread", {"RRRMC_XENTR_NO_WAVE": "1"}, 1), ("std-wave", {"RRRMC_XENTR_WAVE": "1"}, 2)], ids=["thread", "wave"])
def test_standard_mc_follows_the_boltzmann_law(pkg, which, env, build):
    case = BL._case("%s-GraphPercXEntr-5-3-xentr_kernels" % which, None, "std", BL_BETA, BL_ITERS, BL_SEEDS[which], env=env)
    X = bl_graph(pkg)
    E = bl_energies(X)
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))
    with BL.with_env(env), pkg.Engine(X, 2) as eng:                # (the switches name the build the case ran)
        eng.seed(1)
        eng.init_spins_random()
        eng.standard_mc(BL_BETA, 10, 10)
        assert eng.xentr_build() == build


@pytest.mark.parametrize("env", [{}, {"RRRMC_AF_NO_LDS": "1"}], ids=["lds", "global"])
def test_rrr_mc_on_add_sub_fields_follows_the_law_of_g(pkg, env):
    case = BL._case("rrr-GraphAddSubFields-GraphPercXEntr-5-3-af_kernels", None, "rrr", BL_BETA, BL_ITERS, BL_SEEDS["rrr-asf"], env=env)
    g = bl_graph(pkg)
    X = pkg.GraphAddSubFields(bl_fields(), g)
    E = bl_energies(g)
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))
