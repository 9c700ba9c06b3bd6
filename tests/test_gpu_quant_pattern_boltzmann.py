"""GraphQuant over pattern-machine slices against the exact Boltzmann law: 9 spins, 512 states enumerated, both samplers, with the statistic,
thresholds and runner of tests/boltzmann_law.py unchanged.  The slice energies are written here from the reference's definition of the training
error (PercStep.jl:83-111, CommStep.jl:107-141), not taken from the library."""
import numpy as np
import pytest

import boltzmann_law as BL

pytestmark = pytest.mark.gpu

GAMMA, BETA_GRAPH = 0.8, 1.0


def _perc_step_errors(xi):
    """s [S, N] of ±1 -> the number of patterns a with Σ_i ξ_ai s_i < 0 (N odd: never 0)"""
    x = 2 * np.asarray(xi, np.int64) - 1
    return lambda s: ((s @ x.T) < 0).sum(axis=1).astype(np.float64)


def _comm_step_errors(K1, K2, xi):
    """the committee's output Σ_k sign(Σ_(i in unit k) ξ_ai s_i) < 0 (K1, K2 odd: no zeros)"""
    x = 2 * np.asarray(xi, np.int64) - 1

    def f(s):
        out = 0
        for k in range(K2):
            out = out + np.sign(s[:, k * K1:(k + 1) * K1] @ x[:, k * K1:(k + 1) * K1].T)
        return (out < 0).sum(axis=1).astype(np.float64)
    return f


MODELS = {
    "QPercStepT-3-2-3": (lambda pkg: pkg.GraphQPercStepT(3, 2, 3, GAMMA, BETA_GRAPH, seed=21), lambda X: _perc_step_errors(X.X1.patterns())),
    "QCommStepT-3x1-2-3": (lambda pkg: pkg.GraphQCommStepT(3, 1, 2, 3, GAMMA, BETA_GRAPH, seed=22), lambda X: _comm_step_errors(3, 1, X.X1.patterns())),
}


@pytest.mark.parametrize("sampler,iters,seed", [("std", 2700, 171), ("rrr", 1350, 172)])
@pytest.mark.parametrize("model", list(MODELS))
def test_final_configurations_follow_the_boltzmann_law(pkg, model, sampler, iters, seed):
    make, slice_energy = MODELS[model]
    case = BL._case("%s-%s-quant_pat_kernels" % (sampler, model), make, sampler, 0.9, iters, seed)
    X = make(pkg)
    assert X.N == 9
    sg = 2 * BL.enumerate_states(X.N) - 1
    E = BL.energy_quant(slice_energy(X), X.Nk, X.M, X.Gamma, X.beta, sg)
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))
