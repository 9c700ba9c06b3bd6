"""The regular 3-spin model against the exact Boltzmann law: GraphPSpin3(6, 2) (64 states) and GraphPSpin3(9, 1) (512 states) enumerated,
with the statistic, sample counts, thresholds and runner of tests/boltzmann_law.py unchanged (as tests/test_gpu_sat_boltzmann.py uses
them: 65 536 chains, 2700 iterations of standardMC, 1350 of rrrMC).  The energies are written here from the definition — minus the sum
over every layer's triples of the product of the three spins (PSpin3.jl:62-93) — not taken from the library.  standardMC runs on the graph
in both builds; rrrMC on GraphAddSubFields over it, whose stationary law is g's own."""
import numpy as np
import pytest

import boltzmann_law as BL

pytestmark = pytest.mark.gpu


def _minus_triple_products(A):
    """s [S, N] of ±1 -> −Σ_layers Σ_triples σσσ, summed in exact int64 and handed back as Float64 (the engine reports the tracked energy
    so, as it does GraphSAT's); a triple is taken at its smallest site"""
    A = np.asarray(A, np.int64)
    N, K = A.shape[0], A.shape[1] // 2

    def f(s):
        E = np.zeros(len(s), np.int64)
        for k in range(K):
            n = 0
            for i in range(N):
                y, z = A[i, 2 * k], A[i, 2 * k + 1]
                if i < y and i < z:
                    E -= s[:, i] * s[:, y] * s[:, z]
                    n += 1
            assert n == N // 3                                      # the layer is a partition
        return E.astype(np.float64)
    return f


def _g62(pkg):
    return pkg.GraphPSpin3(6, 2, seed=4)


def _g91(pkg):
    return pkg.GraphPSpin3(9, 1, seed=5)


def _fields(N):
    return np.linspace(-0.8, 0.8, N)


MODELS = {"6-2": (_g62, 0.6), "9-1": (_g91, 0.8)}


@pytest.mark.parametrize("build,env", [("pspin_wave_kernel", {"RRRMC_PSPIN_WAVE": "1"}), ("pspin_standard_kernel", {"RRRMC_PSPIN_NO_WAVE": "1"})])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_graph_pspin3_follows_the_boltzmann_law(pkg, name, build, env):
    model, beta = MODELS[name]
    case = BL._case("std-GraphPSpin3-%s-%s" % (name, build), model, "std", beta, 2700, 191, env=env)
    X = model(pkg)
    sg = 2 * BL.enumerate_states(X.N) - 1
    E = _minus_triple_products(X.A)(sg)
    # (6, 2): the product of its four triple products is (Π σ)² = 1, so E ∈ {−4, 0, 4}; (9, 1): three independent triples, E ∈ {−3, −1, 1, 3}
    assert np.unique(E).tolist() == ([-4, 0, 4] if name == "6-2" else [-3, -1, 1, 3])
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_rrr_mc_on_add_sub_fields_follows_the_law_of_g(pkg, name):
    model, beta = MODELS[name]
    wrapped = lambda p: p.GraphAddSubFields(_fields(model(p).N), model(p))
    case = BL._case("rrr-AddSubFields-GraphPSpin3-%s-af_kernels" % name, wrapped, "rrr", beta, 1350, 192)
    X = wrapped(pkg)
    sg = 2 * BL.enumerate_states(X.N) - 1
    E = _minus_triple_products(X.X1.A)(sg)
    idx, Etr, Es_last = BL.run_engine(pkg, case, X)
    BL.assert_tracked_energy(E, idx, Etr)
    BL.assert_verdict(BL.judge(case, E, idx, Es_last))
