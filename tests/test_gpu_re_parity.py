"""GPU parity for the Robust Ensemble (src/graphs/RE.jl; test/runtests.jl:90-92, scripts/scripts.jl:866-963 test_REIsing): rrrMC(X::DoubleGraph)
and standardMC through the HIP kernels equal the plain-Python restatement (tests/re_reference.py) bit for bit — energies, final configuration,
accepted / staged counts, the DeltaECache's classes and set sizes, energy(X, C) and REenergies."""
import os

import numpy as np
import pytest

import re_reference as RE

pytestmark = pytest.mark.gpu


def _graph(pkg, oracle, kind, Nk, M, gamma, beta_g, seed):
    if kind == "empty":
        return pkg.Graph0RE(Nk, M, gamma, beta_g), None
    if kind == "sk":
        X = pkg.GraphSKRE(Nk, M, gamma, beta_g, seed=seed)
        assert (X.J == oracle.gen_sk_binary(Nk, seed)).all()
        return X, X.J
    J = oracle.gen_sk_gauss(Nk, seed)
    return pkg.GraphRobustEnsemble(Nk, M, gamma, beta_g, pkg.GraphSKNormal.from_J(J)), J


def _check_rrr(pkg, oracle, kind, Nk, M, gamma, beta_g, beta, R, iters, step, thr, check_reps=None, calls=1):
    seed = 7340021 + 31 * Nk + M
    X, J = _graph(pkg, oracle, kind, Nk, M, gamma, beta_g, seed)
    N = Nk * M
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        E0 = eng.energy()
        outs = []
        for c in range(calls):          # a second call continues the streams (not the run: resume is off)
            Es, acc, staged = eng.rrr_mc(beta, iters, step, staged_thr=thr)
            outs.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config(), eng.rrr_cache(), eng.run_energy()))
        REs = eng.re_energies()
        Ef = eng.energy()
    for r in (check_reps if check_reps is not None else range(R)):
        s = RE.config_from_chunks(C0.s[r], N)
        assert (RE.chunks_from_config(s) == C0.s[r]).all()
        assert (C0.s[r] == oracle.init_config(seed, r, N)).all()
        assert E0[r] == RE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s)
        for c in range(calls):
            Xr = RE.make_ensemble(Nk, M, gamma, beta_g, kind, J)
            run = RE.RrrRun(Xr, s, beta, seed, oracle, replica=r, it0=c * iters, staged_thr=thr)
            es = run.run(iters, step)
            Es, acc, staged, C1, (pos, sizes), Etr = outs[c]
            assert np.asarray(Es[r]).tolist() == es, (r, c)
            assert acc[r] == run.accepted and staged[r] == run.staged_its, (r, c)
            assert (C1.s[r] == RE.chunks_from_config(s)).all(), (r, c)
            p_ref, sz_ref = run.cache_view()
            assert (pos[r] == p_ref).all() and (sizes[r] == sz_ref).all(), (r, c)
            assert Etr[r] == run.E
        assert Ef[r] == RE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s)
        REr = REs if R == 1 else REs[r]
        assert np.asarray(REr).tolist() == RE.re_energies(Nk, M, kind, J, s)


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
@pytest.mark.parametrize("thr", [0.5, 0.0, 1.0])
def test_rrr_re_runtests_shapes(pkg, oracle, kind, thr):
    # test/runtests.jl:90-92: GraphRobustEnsemble(10, 8, 1.5, 2.0, ...) over GraphEmpty, GraphSK, GraphSKNormal
    _check_rrr(pkg, oracle, kind, 10, 8, 1.5, 2.0, 2.0, 4, 10000, 100, thr)


@pytest.mark.parametrize("kind,Nk,M,R", [("sk", 45, 5, 3), ("skn", 13, 7, 2), ("empty", 37, 7, 70), ("sk", 33, 5, 70)])
def test_rrr_re_odd_M_unaligned_many_replicas(pkg, oracle, kind, Nk, M, R):
    _check_rrr(pkg, oracle, kind, Nk, M, 1.0, 1.0, 1.5, R, 6000, 250, 0.5, check_reps=[0, 1, R - 1] if R > 3 else None, calls=2)


def test_rrr_re_test_reising_geometry(pkg, oracle):
    # scripts.jl:866-963: GraphSKRE(1024, 5, γ = 2, β = 0.4) (3 replicas of the batch, 20 000 iterations)
    _check_rrr(pkg, oracle, "sk", 1024, 5, 2.0, 0.4, 0.4, 3, 20000, 1000, 0.5)


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_rrr_re_lds_and_global_builds_agree(pkg, kind):
    X = pkg.Graph0RE(21, 6, 1.2, 1.0) if kind == "empty" else pkg.GraphSKRE(21, 6, 1.2, 1.0, seed=3) if kind == "sk" else \
        pkg.GraphRobustEnsemble(21, 6, 1.2, 1.0, pkg.GraphSKNormal(21, seed=3))
    res = []
    for env in ({"RRRMC_RE_NO_LDS": "1"}, {"RRRMC_RE_LDS": "1"}):
        old = {k: os.environ.get(k) for k in ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS")}
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


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_standard_re_bit_exact(pkg, oracle, kind):
    Nk, M, gamma, beta_g, beta, R = 11, 5, 1.5, 2.0, 1.2, 3
    seed = 4411 + M
    X, J = _graph(pkg, oracle, kind, Nk, M, gamma, beta_g, seed)
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        Es, acc = eng.standard_mc(beta, 8000, 100)
        C1 = eng.get_config()
    for r in range(R):
        s = RE.config_from_chunks(C0.s[r], Nk * M)
        Xr = RE.make_ensemble(Nk, M, gamma, beta_g, kind, J)
        es, E, a = RE.standard_mc(Xr, s, beta, 8000, 100, seed, oracle, replica=r)
        assert Es[r].tolist() == es and acc[r] == a
        assert (C1.s[r] == RE.chunks_from_config(s)).all()


def test_re_contexts_refuse(pkg):
    import ctypes as C
    L = pkg.lib()
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 10, 2, 0, 4, 0, 0) == 1                   # M > 2 (RE.jl:37)
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 10000, 7, 0, 4, 0, 0) == 3                # N > 65535
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 10, 40, 0, 4, 0, 0) == 3                  # M > 32
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 10, 5, 7, 4, 0, 0) == 1                   # slice kind
    X = pkg.Graph0RE(10, 5, 1.0, 1.0)
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call in (lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0),
                     lambda: eng.extremal_opt(1.4, 100, 10)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3
