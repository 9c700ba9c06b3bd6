"""GPU parity for the Local Entropy ensemble (src/graphs/LE.jl; test/runtests.jl:102-103): rrrMC(X::DoubleGraph) and standardMC through the
HIP kernels equal the plain-Python restatement (tests/le_reference.py) bit for bit — energies, final configuration, accepted / staged counts,
the DeltaECache's classes and set sizes, energy(X, C), LEenergies, cenergy and distances — and the kernels' bounds are enforced."""
import os

import numpy as np
import pytest

import le_reference as LE

pytestmark = pytest.mark.gpu


def _graph(pkg, oracle, kind, Nk, M, gamma, beta_g, seed):
    if kind == "empty":
        return pkg.Graph0LE(Nk, M, gamma, beta_g), None
    if kind == "sk":
        X = pkg.GraphSKLE(Nk, M, gamma, beta_g, seed=seed)
        assert (X.J == oracle.gen_sk_binary(Nk, seed)).all()
        return X, X.J
    J = oracle.gen_sk_gauss(Nk, seed)
    return pkg.GraphLocalEntropy(Nk, M, gamma, beta_g, pkg.GraphSKNormal.from_J(J)), J


def _check_observables(eng, R, Nk, M, kind, J, configs):
    LEs, Ec, D = eng.le_energies(), eng.cenergy(), eng.distances()
    for r, s in configs:
        LEr = LEs if R == 1 else LEs[r]
        Ecr = Ec if R == 1 else Ec[r]
        Dr = D if R == 1 else D[r]
        assert np.asarray(LEr).tolist() == LE.le_energies(Nk, M, kind, J, s)
        assert float(Ecr) == LE.cenergy(Nk, M, kind, J, s)
        assert np.asarray(Dr).tolist() == LE.distances(Nk, M, s)


def _check_rrr(pkg, oracle, kind, Nk, M, gamma, beta_g, beta, R, iters, step, thr, check_reps=None, calls=1):
    seed = 9120041 + 31 * Nk + M
    X, J = _graph(pkg, oracle, kind, Nk, M, gamma, beta_g, seed)
    N = Nk * (M + 1)
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        E0 = eng.energy()
        outs = []
        for c in range(calls):          # a second call continues the streams (not the run: resume is off)
            Es, acc, staged = eng.rrr_mc(beta, iters, step, staged_thr=thr)
            outs.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config(), eng.rrr_cache(), eng.run_energy()))
        reps = list(check_reps if check_reps is not None else range(R))
        finals = {}
        Ef = eng.energy()
        for r in reps:
            s = LE.config_from_chunks(C0.s[r], N)
            assert (C0.s[r] == oracle.init_config(seed, r, N)).all()
            assert E0[r] == LE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s)
            for c in range(calls):
                Xr = LE.make_ensemble(Nk, M, gamma, beta_g, kind, J)
                run = LE.RrrRun(Xr, s, beta, seed, oracle, replica=r, it0=c * iters, staged_thr=thr)
                es = run.run(iters, step)
                Es, acc, staged, C1, (pos, sizes), Etr = outs[c]
                assert np.asarray(Es[r]).tolist() == es, (r, c)
                assert acc[r] == run.accepted and staged[r] == run.staged_its, (r, c)
                assert (C1.s[r] == LE.chunks_from_config(s)).all(), (r, c)
                p_ref, sz_ref = run.cache_view()
                assert (pos[r] == p_ref).all() and (sizes[r] == sz_ref).all(), (r, c)
                assert Etr[r] == run.E
            assert Ef[r] == LE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s)
            finals[r] = s
        _check_observables(eng, R, Nk, M, kind, J, finals.items())


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
@pytest.mark.parametrize("thr", [0.5, 0.0, 1.0])
def test_rrr_le_runtests_shapes(pkg, oracle, kind, thr):
    # test/runtests.jl:102-103: GraphLocalEntropy(10, 8, 1.5, 2.0, ...) over GraphEmpty, GraphSKNormal (and GraphSKLE)
    _check_rrr(pkg, oracle, kind, 10, 8, 1.5, 2.0, 2.0, 4, 10000, 100, thr)


@pytest.mark.parametrize("kind,Nk,M,R,gamma", [("sk", 45, 5, 3, 1.0), ("skn", 13, 7, 2, -0.8), ("empty", 37, 3, 70, 1.0), ("sk", 33, 6, 70, 0.6),
                                               ("skn", 6, 12, 2, 0.4), ("sk", 7, 30, 2, 0.3), ("skn", 9, 4, 3, 0.0)])
def test_rrr_le_odd_even_M_unaligned_many_replicas(pkg, oracle, kind, Nk, M, R, gamma):
    # odd and even M (L from 2 to 17: every class capacity the kernels instantiate), γ of both signs and γ = 0 (repeated zero levels)
    _check_rrr(pkg, oracle, kind, Nk, M, gamma, 1.0, 1.5, R, 6000, 250, 0.5, check_reps=[0, 1, R - 1] if R > 3 else None, calls=2)


def test_rrr_le_skle_bench_geometry(pkg, oracle):
    # GraphSKLE(1024, 5), γ = 2, β = 0.4: the point of profiles/r07/le_skle.md (3 replicas of the batch, 20 000 iterations)
    _check_rrr(pkg, oracle, "sk", 1024, 5, 2.0, 0.4, 0.4, 3, 20000, 1000, 0.5)


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_rrr_le_lds_and_thread_builds_agree(pkg, kind):
    X = pkg.Graph0LE(21, 6, 1.2, 1.0) if kind == "empty" else pkg.GraphSKLE(21, 6, 1.2, 1.0, seed=3) if kind == "sk" else \
        pkg.GraphLocalEntropy(21, 7, 1.2, 1.0, pkg.GraphSKNormal(21, seed=3))
    res = []
    for env in ({"RRRMC_LE_NO_LDS": "1"}, {"RRRMC_LE_LDS": "1"}):
        old = {k: os.environ.get(k) for k in ("RRRMC_LE_NO_LDS", "RRRMC_LE_LDS")}
        os.environ.update(env)
        try:
            with pkg.Engine(X, 5) as eng:
                eng.seed(99)
                eng.init_spins_random()
                out = eng.rrr_mc(1.7, 5000, 50)
                res.append((out, eng.get_config().s.copy(), eng.rrr_cache()))
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    (a, ca, pa), (b, cb, pb) = res
    for x, y in zip(a, b):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert (ca == cb).all() and (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()


@pytest.mark.parametrize("kind,M", [("empty", 5), ("sk", 4), ("skn", 5), ("skn", 8)])
def test_standard_le_bit_exact(pkg, oracle, kind, M):
    Nk, gamma, beta_g, beta, R = 11, 1.5, 2.0, 1.2, 3
    seed = 5511 + M
    X, J = _graph(pkg, oracle, kind, Nk, M, gamma, beta_g, seed)
    N = Nk * (M + 1)
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        Es, acc = eng.standard_mc(beta, 8000, 100)
        C1 = eng.get_config()
        Etr = eng.run_energy()
        finals = []
        for r in range(R):
            s = LE.config_from_chunks(C0.s[r], N)
            Xr = LE.make_ensemble(Nk, M, gamma, beta_g, kind, J)
            es, E, a = LE.standard_mc(Xr, s, beta, 8000, 100, seed, oracle, replica=r)
            assert Es[r].tolist() == es and acc[r] == a
            assert (C1.s[r] == LE.chunks_from_config(s)).all()
            assert Etr[r] == E
            finals.append((r, s))
        _check_observables(eng, R, Nk, M, kind, J, finals)


def test_le_bounds_and_refusals(pkg):
    import ctypes as C
    L = pkg.lib()
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create_le(C.byref(ctx), 10, 2, 0, 4, 0, 0) == 1                   # M > 2 (LE.jl:24)
    assert L.rrrmc_ctx_create_le(C.byref(ctx), 10, 32, 0, 4, 0, 0) == 3                  # M <= 31
    assert L.rrrmc_ctx_create_le(C.byref(ctx), 8192, 7, 0, 4, 0, 0) == 3                 # N = 65 536 > 65 535
    assert L.rrrmc_ctx_create_le(C.byref(ctx), 10, 5, 7, 4, 0, 0) == 1                   # slice kind
    assert L.rrrmc_ctx_create_le(C.byref(ctx), 2047, 31, 0, 1, 0, 0) == 0                # N = 65 504, M = 31: the largest shapes
    L.rrrmc_ctx_destroy(ctx)
    X = pkg.Graph0LE(10, 5, 1.0, 1.0)
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call in (lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0),
                     lambda: eng.extremal_opt(1.4, 100, 10)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3
        assert L.rrrmc_le_set_params(eng._ctx, 1.0, 0.0) == 1                            # γT = γ / β not finite
        assert L.rrrmc_re_set_params(eng._ctx, 1.0, 1.0) == 2                            # not a Robust Ensemble context


def test_le_largest_M_and_N_run(pkg, oracle):
    # M = 31 (L = 16) at N = 2047 * 32 = 65 504 through the thread build, energy tracked against a fresh one
    X = pkg.Graph0LE(2047, 31, 0.9, 1.0)
    with pkg.Engine(X, 2) as eng:
        eng.set_debug_checks(True)
        eng.seed(4)
        eng.init_spins_random()
        eng.rrr_mc(1.0, 3000, 1000)
        eng.standard_mc(1.0, 3000, 1000)
        Etr, E = eng.run_energy(), eng.energy()
        assert (np.abs(Etr - E) <= 1e-10 * np.maximum(1.0, np.abs(E))).all()
