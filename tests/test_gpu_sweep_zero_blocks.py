"""GPU parity of the sweep kernel's zero-block builds (sparse_kernels.hpp: refine_block_zb; the launch picks the build from the leading
all-zero blocks of the thresholds, host_plan.hpp: zero_pattern): energies at every sample, final spins and accepted counts against the
CPU oracle, bit for bit.

Every case runs in the context's own mode (MODE 0 at these sizes) and with the neighbour table forced out of LDS (RRRMC_FORCE_WIDE=1:
MODE 1, the headline's), and each of those a second time through the generic kernel (RRRMC_SWEEP_GENERIC=1, read by the launch code at
every call): the four runs must be identical and equal the oracle's.  K = 3 has a build for every pattern but (0, 0); the other graphs
run the generic kernel either way and pin that nothing else moved.  Which build a launch took is read back (Engine.sweep_build) and
must be the expected one: a selection that always fell back to the generic kernel would fail here."""
import numpy as np
import pytest

from test_gpu_sparse_parity import _graph

pytestmark = pytest.mark.gpu

# beta = 0.3 .. 6.0 at K = 3 give the patterns (0,0), (1,0), (2,0), (3,1), (3,2), (3,3) (tests/test_zero_blocks_cpu.py recomputes them)
BETAS_K3 = [0.3, 0.5, 1.0, 1.5, 3.0, 6.0]
CASES = [(("rrg", N, 3), R, beta, 6000, 64) for N in (64, 256) for R in (32, 40) for beta in BETAS_K3] + [
    (("rrg", 50, 4), 32, 1.0, 6000, 64),
    (("ea", 4, 3), 32, 0.5, 6000, 64),
    (("ea", 4, 3), 32, 1.0, 6000, 64),
    (("circ", 100, 7), 32, 0.3, 5000, 500),     # the circulant K = 7 graph of test_gpu_sparse_parity.py
    (("circ", 100, 7), 32, 1.0, 5000, 500),
]
RUNS = [(wide, generic) for wide in ("0", "1") for generic in ("0", "1")]
# the pattern (two bits per class, class 0 lowest) of the build a K = 3 launch must take in MODE 0 and 1: every pattern has its own build
BUILD_K3 = {0.3: 0, 0.5: 1, 1.0: 2, 1.5: 3 | 1 << 2, 3.0: 3 | 2 << 2, 6.0: 3 | 3 << 2}


def _run(pkg, X, R, seed, beta, iters, step, C0):
    """(Es, acc, final configuration, build of the sweep kernel) of one sampling call on a fresh engine"""
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        assert (eng.get_config().s == C0).all()
        assert eng.sweep_build() == -1                    # no call yet
        Es, acc = eng.standard_mc(beta, iters, step)
        return Es, acc, eng.get_config().s, eng.sweep_build()


@pytest.mark.parametrize("kind,R,beta,iters,step", CASES)
def test_zero_block_builds_bit_exact(pkg, oracle, monkeypatch, kind, R, beta, iters, step):
    seed = 0xBEEF + 11 * kind[1] + R
    X = _graph(pkg, kind, seed)
    A, J = X.A, X.J.astype(np.int32)
    C0 = oracle.init_configs(seed, 0, R, X.N)
    Es_ref, ch_ref, acc_ref = oracle.standard_mc_sparse_batch(A, J, beta, iters, step, seed, C0, form="ea" if kind[0] == "ea" else "rrg")
    for wide, generic in RUNS:
        monkeypatch.setenv("RRRMC_FORCE_WIDE", wide)
        monkeypatch.setenv("RRRMC_SWEEP_GENERIC", generic)
        Es, acc, C1, build = _run(pkg, X, R, seed, beta, iters, step, C0)
        tag = "wide=%s generic=%s" % (wide, generic)
        assert build == (BUILD_K3[beta] if X.K == 3 and generic == "0" else 0), tag
        assert Es.shape == Es_ref.shape, tag
        assert (Es == Es_ref).all(), tag
        assert (C1 == ch_ref).all(), tag
        assert (acc == acc_ref).all(), tag


@pytest.mark.parametrize("wide", ["0", "1"])
def test_pattern_changes_between_queued_calls(pkg, oracle, monkeypatch, wide):
    """Calls of different beta queued back to back on one context, nothing waited for in between: (2,0), then (3,3), then (0,0) — every
    launch picks its own build while the planner and the sweeps of the call before may still be running.  The last call's samples, its
    accepted counts and the final spins are the oracle's, which they can only be if the calls before it were right as well."""
    monkeypatch.setenv("RRRMC_FORCE_WIDE", wide)
    monkeypatch.setenv("RRRMC_SWEEP_GENERIC", "0")
    seed, N, R = 0xFACE, 256, 40
    X = pkg.GraphRRG(N, 3, seed=seed)
    A, J = X.A, X.J.astype(np.int32)
    calls = [(1.0, 5000, 64), (6.0, 4000, 50), (0.3, 3000, 64)]
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config().s
        builds = []
        for beta, iters, step in calls:
            eng.standard_mc_async(beta, iters, step)
            builds.append(eng.sweep_build())
        eng.sync()
        Es, acc = eng.fetch_results()
        C1 = eng.get_config().s
    assert builds == [BUILD_K3[1.0], BUILD_K3[6.0], 0]
    assert (C0 == oracle.init_configs(seed, 0, R, N)).all()
    ch, it0 = C0, 0
    for beta, iters, step in calls:
        Es_ref, ch, acc_ref = oracle.standard_mc_sparse_batch(A, J, beta, iters, step, seed, ch, it0=it0)
        it0 += iters
    assert Es.shape == Es_ref.shape and (Es == Es_ref).all()
    assert (acc == acc_ref).all()
    assert (C1 == ch).all()
