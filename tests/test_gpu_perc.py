"""GPU parity for the binary perceptron (src/graphs/PercStep.jl, PercLinear.jl): standardMC on the stand-alone graphs, and rrrMC /
standardMC on the Robust Ensemble and the Local Entropy ensemble over perceptron slices, equal the plain-Python restatement
(tests/perc_reference.py composed with re_reference / le_reference) bit for bit; the two kernel builds, hooked and resumed runs and
two-shard contexts agree; the debug checks pass; refusals and bounds are enforced; and the final configurations of many chains follow
exp(-β E) / Z exactly (χ², energies from the definition)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import le_reference as LE
import perc_reference as PR
import re_reference as RE

pytestmark = pytest.mark.gpu

ENVS = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS", "RRRMC_LE_NO_LDS", "RRRMC_LE_LDS")


def _graph(pkg, ens, linear, Nk, P, M, gamma, beta_g, seed):
    G = pkg.GraphPercLinear if linear else pkg.GraphPercStep
    X1 = G(Nk, P, seed=seed)
    alias = {("re", False): pkg.GraphPercStepRE, ("re", True): pkg.GraphPercLinearRE, ("le", False): pkg.GraphPercStepLE,
             ("le", True): pkg.GraphPercLinearLE}[(ens, linear)]
    return alias(X1, M, gamma, beta_g), X1.patterns()


def _ref(ens, xi, linear, M, gamma, beta_g):
    return (PR.re_ensemble if ens == "re" else PR.le_ensemble)(xi, linear, M, gamma, beta_g)


def _slice_energies(xi, linear, rows, s):
    return [float(PR.make(xi, linear).energy(np.asarray(s[k::rows], np.int64))) for k in range(rows)]


def _check_observables(eng, ens, R, xi, linear, M, configs):
    if ens == "re":
        Es = eng.re_energies()
        for r, s in configs:
            assert np.asarray(Es if R == 1 else Es[r]).tolist() == _slice_energies(xi, linear, M, s)
        return
    LEs, Ec, D = eng.le_energies(), eng.cenergy(), eng.distances()
    for r, s in configs:
        e = _slice_energies(xi, linear, M + 1, s)
        assert np.asarray(LEs if R == 1 else LEs[r]).tolist() == e[1:]
        assert float(Ec if R == 1 else Ec[r]) == e[0]
        assert np.asarray(D if R == 1 else D[r]).tolist() == LE.distances(xi.shape[1], M, s)


# ---- the stand-alone graphs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("N,P", [(101, 30), (33, 70), (65, 129), (7, 64)])
def test_standalone_standard_mc_bit_exact(pkg, oracle, linear, N, P):
    # (101, 30): test/runtests.jl:69-70; P not a multiple of 64, P > 64, P == 64
    seed, beta, R, iters, step = 771 + N, 1.1, 3, 6000, 100
    X = (pkg.GraphPercLinear if linear else pkg.GraphPercStep)(N, P, seed=seed)
    xi = X.patterns()
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        E0 = eng.energy()
        assert E0.dtype == X.energy_dtype
        Es, acc = eng.standard_mc(beta, iters, step)
        Es2, acc2 = eng.standard_mc(beta, iters, step)          # a second call continues the streams
        C1 = eng.get_config()
        Etr = eng.run_energy()
        for r in range(R):
            s = RE.config_from_chunks(C0.s[r], N)
            Xr = PR.make(xi, linear)
            assert E0[r] == Xr.energy(s)
            es, E, a = PR.standard_mc(Xr, s, beta, iters, step, seed, oracle, replica=r)
            assert Es[r].tolist() == es and acc[r] == a
            es, E, a = PR.standard_mc(PR.make(xi, linear), s, beta, iters, step, seed, oracle, replica=r, it0=iters)
            assert Es2[r].tolist() == es and acc2[r] == a
            assert (C1.s[r] == RE.chunks_from_config(s)).all()
            assert Etr[r] == E


def test_standalone_resumed_sharded_and_hooked(pkg):
    X = pkg.GraphPercLinear(45, 80, seed=9)
    with pkg.Engine(X, 70) as a, pkg.Engine(X, 70) as b, pkg.Engine(X, 70, devices=[0, 0]) as c:
        for e in (a, b, c):
            e.seed(31)
            e.init_spins_random()
        Ea, acca = a.standard_mc(0.9, 3000, 50)
        Ec, accc = c.standard_mc(0.9, 3000, 50)
        b.set_resume(True)
        Es, acc = [], np.zeros(70, np.int64)
        for n in (350, 1, 1649, 1000):
            e_, ac = b.standard_mc(0.9, n, 50)
            Es.append(e_)
            acc += ac
        # the samples of a cut run fall at multiples of `step` of each piece: compare what both took, and the end state
        assert (acca == acc).all() and (acca == accc).all() and (Ea == Ec).all()
        assert (a.get_config().s == b.get_config().s).all() and (a.get_config().s == c.get_config().s).all()
        assert (a.run_energy() == b.run_energy()).all()
    Es0, C0 = pkg.standardMC(X, 0.9, 2000, step=100, seed=5, quiet=True, replicas=3)
    Es1, C1 = pkg.standardMC(X, 0.9, 2000, step=100, seed=5, quiet=True, replicas=3, hook=lambda *a: True)
    assert (np.asarray(Es0) == np.asarray(Es1)).all() and (C0.s == C1.s).all()


def test_standalone_refusals_and_bounds(pkg):
    L = pkg.lib()
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create_perc(C.byref(ctx), 100, 0, 4, 0, 0) == 1                   # N must be odd (PercStep.jl:57)
    assert L.rrrmc_ctx_create_perc(C.byref(ctx), 32769, 0, 4, 0, 0) == 3                 # N <= 32 767
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 100, 5, 3, 4, 0, 0) == 1                  # even Nk under an ensemble
    assert L.rrrmc_ctx_create_le(C.byref(ctx), 100, 5, 4, 4, 0, 0) == 1
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 1001, 31, 3, 1, 0, 0) == 0                # the family's bounds stay: M = 31, N = 31 031
    assert L.rrrmc_set_patterns(ctx, np.zeros(4097 * 16, np.uint64), 4097) == 3          # P <= 4096
    assert L.rrrmc_set_patterns(ctx, np.zeros(16, np.uint64), 0) == 1
    bad = np.zeros(16, np.uint64)
    bad[15] = np.uint64(1) << np.uint64(1001 % 64)
    assert L.rrrmc_set_patterns(ctx, bad, 1) == 1                                        # a bit beyond N
    L.rrrmc_ctx_destroy(ctx)
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 2115, 31, 3, 1, 0, 0) == 3                # N = 65 565 > 65 535
    for X in (pkg.GraphPercStep(11, 5), pkg.GraphPercLinear(11, 5)):
        with pkg.Engine(X, 2) as eng:
            eng.seed(1)
            eng.init_spins_random()
            for call in (lambda: eng.rrr_mc(1.0, 100, 10), lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0),
                         lambda: eng.extremal_opt(1.4, 100, 10)):
                with pytest.raises(pkg.RRRMCError) as e:
                    call()
                assert e.value.code == 3
            assert L.rrrmc_set_couplings_bits(eng._ctx, np.zeros(11, np.uint64)) == 2
    for X in (pkg.GraphPercStepRE(11, 5, 3, 1.0, 1.0), pkg.GraphPercLinearLE(11, 5, 3, 1.0, 1.0)):
        with pkg.Engine(X, 2) as eng:
            eng.seed(1)
            eng.init_spins_random()
            for call in (lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0), lambda: eng.extremal_opt(1.4, 100, 10)):
                with pytest.raises(pkg.RRRMCError) as e:
                    call()
                assert e.value.code == 3
    with pkg.Engine(pkg.Graph0RE(11, 3, 1.0, 1.0), 2) as eng:
        assert L.rrrmc_set_patterns(eng._ctx, np.zeros(5, np.uint64), 5) == 2            # not a perceptron context


# ---- the ensembles ---------------------------------------------------------------------------------------------------------------
def _check_rrr(pkg, oracle, ens, linear, Nk, P, M, gamma, beta_g, beta, R, iters, step, thr, check_reps=None, calls=1):
    seed = 4120041 + 31 * Nk + M
    X, xi = _graph(pkg, ens, linear, Nk, P, M, gamma, beta_g, seed)
    N = X.N
    Ref = RE if ens == "re" else LE
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        E0 = eng.energy()
        outs = []
        for c in range(calls):          # a second call continues the streams (not the run: resume is off)
            Es, acc, staged = eng.rrr_mc(beta, iters, step, staged_thr=thr)
            outs.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config(), eng.rrr_cache(), eng.run_energy()))
        finals = {}
        Ef = eng.energy()
        for r in (check_reps if check_reps is not None else range(R)):
            s = Ref.config_from_chunks(C0.s[r], N)
            assert E0[r] == _ref(ens, xi, linear, M, gamma, beta_g).energy(np.array(s, np.int64))
            for c in range(calls):
                Xr = _ref(ens, xi, linear, M, gamma, beta_g)
                run = Ref.RrrRun(Xr, s, beta, seed, oracle, replica=r, it0=c * iters, staged_thr=thr)
                es = run.run(iters, step)
                Es, acc, staged, C1, (pos, sizes), Etr = outs[c]
                assert np.asarray(Es[r]).tolist() == es, (r, c)
                assert acc[r] == run.accepted and staged[r] == run.staged_its, (r, c)
                assert (C1.s[r] == Ref.chunks_from_config(s)).all(), (r, c)
                p_ref, sz_ref = run.cache_view()
                assert (pos[r] == p_ref).all() and (sizes[r] == sz_ref).all(), (r, c)
                assert Etr[r] == run.E
            assert Ef[r] == _ref(ens, xi, linear, M, gamma, beta_g).energy(np.array(s, np.int64))
            finals[r] = s
        _check_observables(eng, ens, R, xi, linear, M, finals.items())


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("thr", [0.5, 0.0, 1.0])
def test_rrr_ensembles_bit_exact(pkg, oracle, ens, linear, thr):
    _check_rrr(pkg, oracle, ens, linear, 21, 30, 5, 1.5, 2.0, 1.2, 3, 4000, 100, thr)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("linear,Nk,P,M,R", [(False, 15, 70, 4, 70), (True, 9, 129, 6, 3), (False, 33, 64, 3, 2), (True, 13, 7, 8, 70)])
def test_rrr_ensembles_odd_even_M_many_replicas(pkg, oracle, ens, linear, Nk, P, M, R):
    _check_rrr(pkg, oracle, ens, linear, Nk, P, M, 0.7, 1.0, 1.3, R, 3000, 250, 0.5, check_reps=[0, 1, R - 1] if R > 3 else None, calls=2)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("linear,M", [(False, 5), (True, 4)])
def test_standard_ensembles_bit_exact(pkg, oracle, ens, linear, M):
    Nk, P, gamma, beta_g, beta, R = 11, 70, 1.5, 2.0, 1.2, 3
    seed = 5511 + M
    X, xi = _graph(pkg, ens, linear, Nk, P, M, gamma, beta_g, seed)
    Ref = RE if ens == "re" else LE
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        Es, acc = eng.standard_mc(beta, 6000, 100)
        C1 = eng.get_config()
        Etr = eng.run_energy()
        finals = []
        for r in range(R):
            s = Ref.config_from_chunks(C0.s[r], X.N)
            es, E, a = Ref.standard_mc(_ref(ens, xi, linear, M, gamma, beta_g), s, beta, 6000, 100, seed, oracle, replica=r)
            assert Es[r].tolist() == es and acc[r] == a
            assert (C1.s[r] == Ref.chunks_from_config(s)).all()
            assert Etr[r] == E
            finals.append((r, s))
        _check_observables(eng, ens, R, xi, linear, M, finals)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in ENVS}
    for k in ENVS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("linear", [False, True])
def test_lds_and_thread_builds_agree(pkg, ens, linear):
    X, _ = _graph(pkg, ens, linear, 21, 130, 6, 1.2, 1.0, 3)
    up = ens.upper()

    def run():
        with pkg.Engine(X, 37) as eng:
            eng.set_debug_checks(True)
            eng.seed(99)
            eng.init_spins_random()
            out = eng.rrr_mc(1.7, 5000, 50) + eng.rrr_mc(1.7, 3000, 50, staged_thr=1.0)
            return out, eng.get_config().s.copy(), eng.rrr_cache()

    (a, ca, pa), (b, cb, pb) = _with_env({"RRRMC_%s_NO_LDS" % up: "1"}, run), _with_env({"RRRMC_%s_LDS" % up: "1"}, run)
    for x, y in zip(a, b):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert (ca == cb).all() and (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hooked_run_equals_unhooked_and_observables_in_hook(pkg, ens, linear, sampler):
    Nk, P, M, beta, iters, step, R = 13, 40, 5, 1.3, 2000, 100, 3
    X, xi = _graph(pkg, ens, linear, Nk, P, M, 1.5, 2.0, 23)
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    seen = []

    def hook(it, X_, Cfg, acc, E):
        rows = M if ens == "re" else M + 1
        obs = pkg.REenergies(X_) if ens == "re" else np.concatenate([pkg.cenergy(X_)[:, None], pkg.LEenergies(X_)], axis=1)
        assert obs.shape == (R, rows)
        for r in range(R):
            s = RE.config_from_chunks(Cfg.s[r], X_.N)
            assert obs[r].tolist() == _slice_energies(xi, linear, rows, s)          # the per-replica training error
            if ens == "le":
                assert pkg.distances(X_)[r].tolist() == LE.distances(Nk, M, s)
        seen.append(it)
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all()
    assert (C0.s == C1.s).all()


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("linear", [False, True])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, ens, linear):
    R, beta, step, total = 4, 1.1, 50, 3000
    X, _ = _graph(pkg, ens, linear, 9, 70, 6, 1.5, 2.0, 4)
    rng = np.random.default_rng(12)
    cuts = sorted(set(rng.integers(1, total, 7).tolist()))
    pieces = np.diff([0] + cuts + [total]).tolist()
    with pkg.Engine(X, R) as a, pkg.Engine(X, R) as b:
        for e in (a, b):
            e.set_debug_checks(True)
            e.seed(31)
            e.init_spins_random()
        Ea, acca, sta = a.rrr_mc(beta, total, step)
        b.set_resume(True)
        Es, acc, st = [], np.zeros(R, np.int64), np.zeros(R, np.int64)
        for n in pieces:
            e_, ac, s_ = b.rrr_mc(beta, n, step)
            Es.append(e_)
            acc += ac
            st += s_
        assert (Ea == np.concatenate(Es, axis=1)).all() and (acca == acc).all() and (sta == st).all()
        assert (a.get_config().s == b.get_config().s).all()
        pa, pb = a.rrr_cache(), b.rrr_cache()
        assert (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
        assert (a.run_energy() == b.run_energy()).all()


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("linear", [False, True])
def test_two_shard_context_equals_single(pkg, ens, linear):
    X, _ = _graph(pkg, ens, linear, 21, 70, 5, 2.0, 0.4, 2)
    res = []
    for devices in (None, [0, 0]):
        with pkg.Engine(X, 70, devices=devices) as eng:
            eng.seed(5)
            eng.init_spins_random()
            r1 = eng.rrr_mc(0.8, 3000, 100)
            cache = eng.rrr_cache()
            r2 = eng.standard_mc(0.8, 3000, 100)
            obs = (eng.re_energies(),) if ens == "re" else (eng.le_energies(), eng.cenergy(), eng.distances())
            res.append(r1 + r2 + cache + (eng.get_config().s.copy(),) + obs)
    for x, y in zip(*res):
        assert (np.asarray(x) == np.asarray(y)).all()


def test_largest_required_shape_runs_in_both_builds(pkg):
    # Nk = 1001, P = 700 (the shape the kernels' limits must admit), M = 5: tracked energy against a fresh one, debug checks on
    for X in (pkg.GraphPercStepRE(1001, 700, 5, 1.0, 2.0), pkg.GraphPercLinearLE(1001, 700, 5, 1.0, 2.0)):
        for env in ({"RRRMC_RE_NO_LDS": "1", "RRRMC_LE_NO_LDS": "1"}, {"RRRMC_RE_LDS": "1", "RRRMC_LE_LDS": "1"}):
            def run():
                with pkg.Engine(X, 2) as eng:
                    eng.set_debug_checks(True)
                    eng.seed(4)
                    eng.init_spins_random()
                    eng.rrr_mc(2.0, 3000, 1000)
                    eng.standard_mc(2.0, 3000, 1000)
                    Etr, E = eng.run_energy(), eng.energy()
                    assert (np.abs(Etr - E) <= 1e-10 * np.maximum(1.0, np.abs(E))).all()
            _with_env(env, run)


# ---- the stationary distribution ---------------------------------------------------------------------------------------------------
def _energy_from_definition(xi, linear, M, gamma, beta_g, s):
    """E = -Σ_i log(2 cosh(γ μ_i)) / β + Σ_k E_k, with E_k the training error of replica k from the definition: pattern a is misclassified
    when Σ_i σ_i ξ_ai < 0 (ξ = ±1, the pattern's label absorbed); step: their number, linear: 2 Σ ((−Δ − 1) ÷ 2 + 1) / √N"""
    xi = np.asarray(xi, np.int64)
    P, Nk = xi.shape
    sg = 2 * np.asarray(s, np.int64).reshape(Nk, M) - 1
    E = -sum(np.log(2 * np.cosh(gamma * sg[i].sum())) / beta_g for i in range(Nk))
    for k in range(M):
        for a in range(P):
            d = int((sg[:, k] * (2 * xi[a] - 1)).sum())
            if d < 0:
                E += 2 * ((-d - 1) // 2 + 1) / np.sqrt(Nk) if linear else 1
    return E


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_final_configurations_follow_the_boltzmann_distribution(pkg, linear, sampler):
    # GraphRobustEnsemble(3, 3, γ = 0.6, β = 1.2) over a perceptron with Nk = 3, P = 2: N = 9, 512 states; 65 536 chains, one final each
    Nk, P, M, gamma, beta_g, beta, R = 3, 2, 3, 0.6, 1.2, 0.6, 65536
    X1 = (pkg.GraphPercLinear if linear else pkg.GraphPercStep)(Nk, P, seed=22)       # (smallest expected count: 83.1 step, 15.5 linear)
    X = pkg.GraphRobustEnsemble(Nk, M, gamma, beta_g, X1)
    xi = X1.patterns()
    N = X.N
    states = list(itertools.product((0, 1), repeat=N))
    E = np.array([_energy_from_definition(xi, linear, M, gamma, beta_g, s) for s in states])
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    expected = p * R
    assert expected.min() >= 5                         # every bin is a valid χ² term
    with pkg.Engine(X, R) as eng:
        eng.seed(424242)
        eng.init_spins_random()
        if sampler == "rrr":
            eng.rrr_mc(beta, 4000, 4000)
        else:
            eng.standard_mc(beta, 4000, 4000)
        Cfg = eng.get_config()
        idx = np.zeros(R, np.int64)
        for j in range(N):                             # state index: site 0 is the most significant bit, as itertools.product orders them
            idx = idx * 2 + ((Cfg.s[:, 0] >> np.uint64(j)) & np.uint64(1)).astype(np.int64)
        assert np.abs(eng.run_energy() - E[idx]).max() < 1e-12
    counts = np.bincount(idx, minlength=len(states))
    stat = float(((counts - expected) ** 2 / expected).sum())
    # the χ² quantile of the 1e-6 upper tail, Wilson-Hilferty (z = 4.7534 is the normal 1e-6 quantile)
    k = len(states) - 1
    limit = k * (1 - 2 / (9 * k) + 4.753424 * (2 / (9 * k)) ** 0.5) ** 3
    assert stat < limit, (stat, limit)
