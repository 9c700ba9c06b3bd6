"""The inputs and the matrix of tests/test_gpu_pm1_builds.py, checked without a GPU: every graph shape is a valid instance that the oracle
runs (random-site chain and colour sweeps, both verdicts exercised), the algorithm of the sweep kernel (tests/emulate_sweep.py) equals the
oracle on the complete graphs — one slot per level, as many levels as the chunk is long — and the parameter lists of the GPU tests are
the full cross products: no cell can be dropped silently."""
import numpy as np
import pytest

import emulate_sweep as EM
import pm1_instances as PI


@pytest.mark.parametrize("shape", PI.all_graph_shapes())
def test_numpy_graphs_are_valid_and_the_oracle_runs_them(oracle, shape):
    A, J8 = PI.graph(shape)
    PI.check_graph(A, J8)
    A, J = np.array(A), np.array(J8, np.int32)
    N, K = A.shape
    assert N == (shape[1] + 1 if shape[0] == "complete" else shape[1]) and K == shape[-1]
    seed, R, beta = 77 + N + K, 3, 0.7
    iters, step = (3000, 100) if N < 1000 else (12000, 1000)
    ch = oracle.init_configs(seed, 0, R, N)
    Es, ch1, acc = oracle.standard_mc_sparse_batch(A, J, beta, iters, step, seed, ch)
    assert Es.shape == (R, iters // step)
    assert (acc > 0.05 * iters).all() and (acc < 0.95 * iters).all()            # both verdicts
    for r in range(R):
        assert Es[r, 0] == oracle.standard_mc_sparse(A, J, beta, step, step, seed, ch[r], replica=r)[0][0]
        one = oracle.standard_mc_sparse(A, J, beta, iters, step, seed, ch[r], replica=r)
        assert (one[0] == Es[r]).all() and (one[1] == ch1[r]).all() and one[2] == acc[r]
        assert (one[3] == oracle.sparse_energy(A, J, ch1[r], want_fields=True)[1]).all()
    # colour sweeps: one colour per site on the complete graphs (what the GPU test uses), greedy otherwise
    color = np.arange(N, dtype=np.int32) if shape[0] == "complete" else oracle.greedy_coloring(A)
    assert (color[A] != color[:, None]).all()                                    # proper
    sweeps = 12 if N < 1000 else 3
    Ec, chc, accc = oracle.colored_sweeps_sparse(A, J, color, beta, sweeps, 1, seed, ch[0], replica=0)
    assert len(Ec) == sweeps and 0 < accc < sweeps * N
    Ec2, chc2, _ = oracle.colored_sweeps_sparse(A, J, color, beta, 1, 1, seed, chc, sweep0=sweeps, replica=0)
    assert Ec2[0] == oracle.sparse_energy(A, J, chc)


@pytest.mark.parametrize("LD", sorted({c[0] for c in PI.CASES_D} | {(1025, 2)}))
def test_lattices_of_the_size_limit(oracle, LD):
    """GraphEA(1024, 2), GraphEA(80, 3) and the refused GraphEA(1025, 2): the sizes the GPU test relies on, and a short oracle run."""
    L_, D = LD
    A = oracle.gen_ea(L_, D)
    N = A.shape[0]
    assert (N, A.shape[1]) == {(1024, 2): (1 << 20, 4), (80, 3): (512000, 6), (1025, 2): (1050625, 4)}[LD]
    J = oracle.gen_couplings(A, 5)
    ch = oracle.init_config(5, 0, N)
    Es, ch1, acc, _ = oracle.standard_mc_sparse(A, J, 0.35, 2000, 500, 5, ch, form="ea")
    assert 0 < acc < 2000 and Es[-1] != Es[0]
    if L_ % 2 == 0:                                   # (an odd L has no checkerboard; the GPU test only asks that lattice for its refusal)
        color = oracle.checkerboard_coloring(L_, D)
        Ec, _, accc = oracle.colored_sweeps_sparse(A, J, color, 0.35, 1, 1, 5, ch)
        assert 0 < accc < N


@pytest.mark.parametrize("K", PI.KS)
def test_sweep_algorithm_on_complete_graphs(oracle, K):
    """The level schedule at its deepest: every attempt is a level of its own."""
    A, J8 = PI.graph(("complete", K))
    A, J = np.array(A), np.array(J8, np.int32)
    N, R, seed, beta, iters, step = K + 1, 32, 900 + K, 0.7, 300, 7
    order, vecs = EM.plan_chunk([oracle.site_of(seed, g, N) for g in range(1, 65)], A)
    assert len(vecs) == 64 and all(n == 1 for _, n in vecs) and list(order) == list(range(64))
    ch = oracle.init_configs(seed, 0, R, N)
    Es, ch2, acc = oracle.standard_mc_sparse_batch(A, J, beta, iters, step, seed, ch)

    def slice_bits(chunks):
        return [sum(((int(chunks[r, x >> 6]) >> (x & 63)) & 1) << r for r in range(R)) for x in range(N)]

    Es2, sp2, acc2 = EM.sweep(oracle.philox, oracle.site_of, oracle.threshold, A, J, beta, iters, step, seed, slice_bits(ch), C=128)
    assert sp2 == slice_bits(ch2)
    assert (np.array(Es2).T == Es).all()
    assert (np.array(acc2) == acc).all() and 0 < acc.min() and acc.max() < iters


def _params(fn):
    marks = [m for m in fn.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1
    return [tuple(p) if isinstance(p, (tuple, list)) else p for p in marks[0].args[1]]


def test_gpu_matrix_is_the_full_cross_product():
    import test_gpu_pm1_builds as G
    want = PI.expected_products()
    got = {"a": _params(G.test_every_degree_on_every_path), "b": _params(G.test_long_levels), "c": _params(G.test_replicas_per_workgroup),
           "d": _params(G.test_size_limit), "e": _params(G.test_colour_sweeps_every_degree), "f": _params(G.test_call_shapes_on_every_path)}
    for k in "abcdef":
        assert len(set(got[k])) == len(got[k]), k                     # no cell twice
        assert sorted(got[k], key=repr) == sorted(want[k], key=repr), k
    assert [len(got[k]) for k in "abcdef"] == [84, 14, 42, 4, 28, 24]
    # every path value of rrrmc_sweep_layout is asked for at every K: 0..3, 4 and 6 by (a), 5 and 4 by (c), 7 and 8 by (e)
    for K in PI.KS:
        asked = {PI.PATHS[p][1] for k, p, _ in got["a"] if k == K} | {PI.big_path(k, l) for k, l in got["c"] if k == K} | \
                {8 if c else 7 for k, c, _ in got["e"] if k == K}
        assert asked == set(range(9)), (K, asked)
    # no case is marked skip / xfail
    for fn in (G.test_every_degree_on_every_path, G.test_long_levels, G.test_replicas_per_workgroup, G.test_size_limit,
               G.test_colour_sweeps_every_degree, G.test_call_shapes_on_every_path):
        assert {m.name for m in fn.pytestmark} == {"parametrize"}
    assert [m.name for m in G.pytestmark] == ["gpu"] if isinstance(G.pytestmark, list) else G.pytestmark.name == "gpu"


def test_compact_mask_rule():
    """the documented rule, spelled out: one mask word per (slot, workgroup) where NT << lgr <= 32 and lgr <= 4"""
    table = {K: [PI.big_path(K, l) for l in range(6)] for K in PI.KS}
    assert table[1] == table[2] == [5, 5, 5, 5, 5, 4]
    assert table[3] == table[4] == [5, 5, 5, 5, 5, 4]
    assert table[5] == table[6] == [5, 5, 5, 5, 4, 4]
    assert table[7] == [5, 5, 5, 5, 4, 4]
