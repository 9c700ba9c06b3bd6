"""GPU parity for the binary committee machines (src/graphs/CommStep.jl, CommReLU.jl): standardMC on the stand-alone graphs, and rrrMC /
standardMC on the Robust Ensemble and the Local Entropy ensemble over committee slices, equal the plain-Python restatement
(tests/comm_reference.py composed with re_reference / le_reference) bit for bit; a committee with one hidden unit is the perceptron, bit for
bit; the two kernel builds, hooked and resumed runs and two-shard contexts agree; the debug checks pass; refusals and bounds are enforced;
and the final configurations of many chains follow exp(-β E) / Z exactly (χ², energies from the definition)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import comm_reference as CR
import le_reference as LE
import re_reference as RE

pytestmark = pytest.mark.gpu

ENVS = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS", "RRRMC_LE_NO_LDS", "RRRMC_LE_LDS")
RUNTESTS = [(False, 25, 5, 30, False), (False, 21, 5, 30, True), (True, 24, 6, 30, False), (True, 22, 6, 30, True)]   # test/runtests.jl:72-75


def _G(pkg, relu):
    return pkg.GraphCommReLU if relu else pkg.GraphCommStep


def _graph(pkg, ens, relu, K1, K2, P, M, gamma, beta_g, seed, fc=False):
    X1 = _G(pkg, relu)(K1, K2, P, fc=fc, seed=seed)
    alias = {("re", False): pkg.GraphCommStepRE, ("re", True): pkg.GraphCommReLURE, ("le", False): pkg.GraphCommStepLE,
             ("le", True): pkg.GraphCommReLULE}[(ens, relu)]
    return alias(X1, M, gamma, beta_g), X1


def _ref(ens, X1, M, gamma, beta_g):
    return (CR.re_ensemble if ens == "re" else CR.le_ensemble)(X1.K2, X1.patterns(), X1.labels(), M, gamma, beta_g)


def _slice_energies(X1, rows, s):
    return [float(CR.energy_from_definition(X1.K2, X1.patterns(), X1.labels(), np.asarray(s[k::rows], np.int64))) for k in range(rows)]


def _check_observables(eng, ens, R, X1, M, configs):
    if ens == "re":
        Es = eng.re_energies()
        for r, s in configs:
            assert np.asarray(Es if R == 1 else Es[r]).tolist() == _slice_energies(X1, M, s)
        return
    LEs, Ec, D = eng.le_energies(), eng.cenergy(), eng.distances()
    for r, s in configs:
        e = _slice_energies(X1, M + 1, s)
        assert np.asarray(LEs if R == 1 else LEs[r]).tolist() == e[1:]
        assert float(Ec if R == 1 else Ec[r]) == e[0]
        assert np.asarray(D if R == 1 else D[r]).tolist() == LE.distances(X1.N, M, s)


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


# ---- the stand-alone graphs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu,K1,K2,P,fc", RUNTESTS + [(False, 7, 3, 64, False), (True, 4, 4, 129, True)])
def test_standalone_standard_mc_bit_exact(pkg, oracle, relu, K1, K2, P, fc):
    seed, beta, R, iters, step = 913 + K1 * K2, 1.1, 3, 3000, 100
    X = _G(pkg, relu)(K1, K2, P, fc=fc, seed=seed)
    xi, y = X.patterns(), X.labels()
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
            s = RE.config_from_chunks(C0.s[r], X.N)
            assert E0[r] == CR.make(K2, xi, y).energy(s)
            es, E, a = CR.standard_mc(CR.make(K2, xi, y), s, beta, iters, step, seed, oracle, replica=r)
            assert Es[r].tolist() == es and acc[r] == a
            es, E, a = CR.standard_mc(CR.make(K2, xi, y), s, beta, iters, step, seed, oracle, replica=r, it0=iters)
            assert Es2[r].tolist() == es and acc2[r] == a
            assert (C1.s[r] == RE.chunks_from_config(s)).all()
            assert Etr[r] == E


def test_one_hidden_unit_is_the_perceptron(pkg):
    # GraphCommStep.from_patterns(1, ξ) and GraphPercStep.from_patterns(ξ): same streams, same integer ΔE, so the same bits
    xi = np.random.default_rng(5).integers(0, 2, (70, 45))
    Cm, Pc = pkg.GraphCommStep.from_patterns(1, xi), pkg.GraphPercStep.from_patterns(xi)
    outs = []
    for X in (Cm, Pc):
        with pkg.Engine(X, 67) as eng:
            eng.set_debug_checks(True)
            eng.seed(8)
            eng.init_spins_random()
            outs.append(eng.standard_mc(0.9, 4000, 100) + eng.standard_mc(0.9, 1000, 100) + (eng.get_config().s.copy(), eng.run_energy()))
    for a, b in zip(*outs):
        assert (np.asarray(a) == np.asarray(b)).all()
    for ens in (pkg.GraphRobustEnsemble, pkg.GraphLocalEntropy):
        outs = []
        for X1 in (Cm, Pc):
            with pkg.Engine(ens(45, 5, 0.5, 2.0, X1), 5) as eng:
                eng.set_debug_checks(True)
                eng.seed(9)
                eng.init_spins_random()
                outs.append(eng.rrr_mc(1.3, 3000, 100) + eng.standard_mc(1.3, 2000, 100) + (eng.get_config().s.copy(), eng.run_energy()))
        for a, b in zip(*outs):
            assert (np.asarray(a) == np.asarray(b)).all()


def test_standalone_resumed_sharded_and_hooked(pkg):
    X = pkg.GraphCommReLU(6, 4, 80, seed=9)
    with pkg.Engine(X, 70) as a, pkg.Engine(X, 70) as b, pkg.Engine(X, 70, devices=[0, 0]) as c:
        for e in (a, b, c):
            e.seed(31)
            e.init_spins_random()
        Ea, acca = a.standard_mc(0.9, 3000, 50)
        Ec, accc = c.standard_mc(0.9, 3000, 50)
        b.set_resume(True)
        acc = np.zeros(70, np.int64)
        for n in (350, 1, 1649, 1000):
            acc += b.standard_mc(0.9, n, 50)[1]
        assert (acca == acc).all() and (acca == accc).all() and (Ea == Ec).all()
        assert (a.get_config().s == b.get_config().s).all() and (a.get_config().s == c.get_config().s).all()
        assert (a.run_energy() == b.run_energy()).all()
    Es0, C0 = pkg.standardMC(X, 0.9, 2000, step=100, seed=5, quiet=True, replicas=3)
    Es1, C1 = pkg.standardMC(X, 0.9, 2000, step=100, seed=5, quiet=True, replicas=3, hook=lambda *a: True)
    assert (np.asarray(Es0) == np.asarray(Es1)).all() and (C0.s == C1.s).all()


def test_refusals_and_bounds(pkg):
    L = pkg.lib()
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create_comm(C.byref(ctx), 4, 3, 0, 4, 0, 0) == 1                   # K1 must be odd (CommStep.jl:65)
    assert L.rrrmc_ctx_create_comm(C.byref(ctx), 3, 4, 0, 4, 0, 0) == 1                   # K2 must be odd
    assert L.rrrmc_ctx_create_comm(C.byref(ctx), 3, 2, 1, 4, 0, 0) == 1                   # K1 must be even (CommReLU.jl:68)
    assert L.rrrmc_ctx_create_comm(C.byref(ctx), 4, 3, 1, 4, 0, 0) == 1                   # K2 must be even
    assert L.rrrmc_ctx_create_comm(C.byref(ctx), 32769, 1, 0, 4, 0, 0) == 3               # N <= 32 767
    assert L.rrrmc_ctx_create_comm(C.byref(ctx), 8194, 4, 1, 4, 0, 0) == 3
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 100, 5, 5, 4, 0, 0) == 1                   # even Nk for a step committee
    assert L.rrrmc_ctx_create_le(C.byref(ctx), 30, 5, 6, 4, 0, 0) == 1                    # Nk % 4 != 0 for a ReLU committee
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 1005, 31, 5, 1, 0, 0) == 0                 # the family's bounds stay: M = 31, N = 31 155
    xi = np.zeros(4097 * 16, np.uint64)
    assert L.rrrmc_set_comm_patterns(ctx, 5, xi, None, 4097) == 3                          # P <= 4096
    assert L.rrrmc_set_comm_patterns(ctx, 5, xi, None, 0) == 1
    assert L.rrrmc_set_comm_patterns(ctx, 4, xi, None, 5) == 1                             # N % K2 != 0
    assert L.rrrmc_set_comm_patterns(ctx, 5, xi, np.zeros(1, np.uint64), 5) == 1           # an extra y
    bad = np.zeros(16, np.uint64)
    bad[15] = np.uint64(1) << np.uint64(1005 % 64)
    assert L.rrrmc_set_comm_patterns(ctx, 5, bad, None, 1) == 1                            # a bit beyond N
    assert L.rrrmc_set_patterns(ctx, np.zeros(16, np.uint64), 1) == 2                      # not a perceptron context
    L.rrrmc_ctx_destroy(ctx)
    assert L.rrrmc_ctx_create_re(C.byref(ctx), 2115, 31, 5, 1, 0, 0) == 3                 # N = 65 565 > 65 535
    assert L.rrrmc_ctx_create_le(C.byref(ctx), 8, 5, 6, 2, 0, 0) == 0
    assert L.rrrmc_set_comm_patterns(ctx, 2, np.zeros(3, np.uint64), None, 3) == 1         # a missing y
    assert L.rrrmc_set_comm_patterns(ctx, 1, np.zeros(3, np.uint64), np.zeros(1, np.uint64), 3) == 1      # K2 = 1 is odd
    assert L.rrrmc_set_comm_patterns(ctx, 2, np.zeros(3, np.uint64), np.full(1, 8, np.uint64), 3) == 1    # a label bit beyond P
    assert L.rrrmc_set_comm_patterns(ctx, 2, np.zeros(3, np.uint64), np.zeros(1, np.uint64), 3) == 0
    L.rrrmc_ctx_destroy(ctx)
    for X in (pkg.GraphCommStep(3, 3, 5), pkg.GraphCommReLU(2, 4, 5)):
        with pkg.Engine(X, 2) as eng:
            eng.seed(1)
            eng.init_spins_random()
            assert L.rrrmc_set_comm_patterns(eng._ctx, X.K2 + 2, X.xi.reshape(-1), X.y, 5) == 1      # not the context's K2
            for call in (lambda: eng.rrr_mc(1.0, 100, 10), lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0),
                         lambda: eng.extremal_opt(1.4, 100, 10)):
                with pytest.raises(pkg.RRRMCError) as e:
                    call()
                assert e.value.code == 3
    for X in (pkg.GraphCommStepRE(3, 3, 5, 3, 1.0, 1.0), pkg.GraphCommReLULE(2, 4, 5, 3, 1.0, 1.0)):
        with pkg.Engine(X, 2) as eng:
            eng.seed(1)
            eng.init_spins_random()
            for call in (lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0), lambda: eng.extremal_opt(1.4, 100, 10)):
                with pytest.raises(pkg.RRRMCError) as e:
                    call()
                assert e.value.code == 3
    with pkg.Engine(pkg.GraphPercStepRE(11, 5, 3, 1.0, 1.0), 2) as eng:
        assert L.rrrmc_set_comm_patterns(eng._ctx, 1, np.zeros(5, np.uint64), None, 5) == 2     # not a committee context


# ---- the ensembles ---------------------------------------------------------------------------------------------------------------
def _check_rrr(pkg, oracle, ens, relu, K1, K2, P, M, gamma, beta_g, beta, R, iters, step, thr, fc=False, check_reps=None, calls=1):
    seed = 51301 + 31 * K1 * K2 + M
    X, X1 = _graph(pkg, ens, relu, K1, K2, P, M, gamma, beta_g, seed, fc)
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
            assert E0[r] == _ref(ens, X1, M, gamma, beta_g).energy(np.array(s, np.int64))
            for c in range(calls):
                run = Ref.RrrRun(_ref(ens, X1, M, gamma, beta_g), s, beta, seed, oracle, replica=r, it0=c * iters, staged_thr=thr)
                es = run.run(iters, step)
                Es, acc, staged, C1, (pos, sizes), Etr = outs[c]
                assert np.asarray(Es[r]).tolist() == es, (r, c)
                assert acc[r] == run.accepted and staged[r] == run.staged_its, (r, c)
                assert (C1.s[r] == Ref.chunks_from_config(s)).all(), (r, c)
                p_ref, sz_ref = run.cache_view()
                assert (pos[r] == p_ref).all() and (sizes[r] == sz_ref).all(), (r, c)
                assert Etr[r] == run.E
            assert Ef[r] == _ref(ens, X1, M, gamma, beta_g).energy(np.array(s, np.int64))
            finals[r] = s
        _check_observables(eng, ens, R, X1, M, finals.items())


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("relu,K1,K2,P,fc", RUNTESTS)
def test_rrr_ensembles_runtests_shapes_bit_exact(pkg, oracle, ens, relu, K1, K2, P, fc):
    # test/runtests.jl:96-99, 108-111: M = 5, γ = 0.5, β = 2.0
    _check_rrr(pkg, oracle, ens, relu, K1, K2, P, 5, 0.5, 2.0, 2.0, 2, 2000, 100, 0.5, fc=fc)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("thr", [0.0, 1.0])
def test_rrr_ensembles_staged_thresholds(pkg, oracle, ens, relu, thr):
    K1, K2 = (4, 2) if relu else (3, 3)
    _check_rrr(pkg, oracle, ens, relu, K1, K2, 40, 5, 1.5, 2.0, 1.2, 3, 3000, 100, thr)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("relu,K1,K2,P,M,R", [(False, 5, 3, 70, 4, 70), (True, 2, 4, 129, 6, 3), (False, 3, 5, 64, 3, 2), (True, 4, 2, 7, 7, 70)])
def test_rrr_ensembles_odd_even_M_many_replicas(pkg, oracle, ens, relu, K1, K2, P, M, R):
    _check_rrr(pkg, oracle, ens, relu, K1, K2, P, M, 0.7, 1.0, 1.3, R, 2500, 250, 0.5, check_reps=[0, 1, R - 1] if R > 3 else None, calls=2)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("relu,K1,K2,P,fc,M", [RUNTESTS[0] + (5,), RUNTESTS[3] + (5,), (True, 4, 2, 70, False, 4), (False, 3, 3, 70, False, 3)])
def test_standard_ensembles_bit_exact(pkg, oracle, ens, relu, K1, K2, P, fc, M):
    gamma, beta_g, beta, R = 0.5, 2.0, 1.2, 3
    seed = 5511 + M + K1
    X, X1 = _graph(pkg, ens, relu, K1, K2, P, M, gamma, beta_g, seed, fc)
    Ref = RE if ens == "re" else LE
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        outs = [eng.standard_mc(beta, 2000, 100) + (eng.get_config(), eng.run_energy()) for _ in range(2)]
        finals = []
        for r in range(R):
            s = Ref.config_from_chunks(C0.s[r], X.N)
            for c, (Es, acc, C1, Etr) in enumerate(outs):
                es, E, a = Ref.standard_mc(_ref(ens, X1, M, gamma, beta_g), s, beta, 2000, 100, seed, oracle, replica=r, it0=2000 * c)
                assert Es[r].tolist() == es and acc[r] == a
                assert (C1.s[r] == Ref.chunks_from_config(s)).all()
                assert Etr[r] == E
            finals.append((r, s))
        _check_observables(eng, ens, R, X1, M, finals)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("relu", [False, True])
def test_lds_and_thread_builds_agree(pkg, ens, relu):
    X, _ = _graph(pkg, ens, relu, 6 if relu else 7, 4 if relu else 3, 130, 6, 1.2, 1.0, 3)
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
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hooked_run_equals_unhooked_and_observables_in_hook(pkg, ens, relu, sampler):
    M, beta, iters, step, R = 5, 1.3, 2000, 100, 3
    X, X1 = _graph(pkg, ens, relu, 4 if relu else 3, 2 if relu else 3, 40, M, 1.5, 2.0, 23)
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    seen = []

    def hook(it, X_, Cfg, acc, E):
        rows = M if ens == "re" else M + 1
        obs = pkg.REenergies(X_) if ens == "re" else np.concatenate([pkg.cenergy(X_)[:, None], pkg.LEenergies(X_)], axis=1)
        assert obs.shape == (R, rows)
        for r in range(R):
            s = RE.config_from_chunks(Cfg.s[r], X_.N)
            assert obs[r].tolist() == _slice_energies(X1, rows, s)          # the per-replica training error
            if ens == "le":
                assert pkg.distances(X_)[r].tolist() == LE.distances(X1.N, M, s)
        seen.append(it)
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all()
    assert (C0.s == C1.s).all()


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("relu", [False, True])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, ens, relu):
    R, beta, step, total = 4, 1.1, 50, 3000
    X, _ = _graph(pkg, ens, relu, 2 if relu else 3, 4 if relu else 3, 70, 6, 1.5, 2.0, 4)
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
@pytest.mark.parametrize("relu", [False, True])
def test_two_shard_context_equals_single(pkg, ens, relu):
    X, _ = _graph(pkg, ens, relu, 6 if relu else 7, 2 if relu else 3, 70, 5, 2.0, 0.4, 2)
    res = []
    for devices in (None, [0, 0]):
        with pkg.Engine(X, 70, devices=devices) as eng:
            eng.seed(5)
            eng.init_spins_random()
            r1 = eng.rrr_mc(0.8, 3000, 100)
            cache = eng.rrr_cache()
            r2 = eng.standard_mc(0.8, 3000, 100)
            obs = (eng.re_energies(),) if ens == "re" else (eng.le_energies(), eng.cenergy(), eng.distances())
            res.append(r1 + r2 + cache + (eng.get_config().s.copy(), eng.energy()) + obs)
    for x, y in zip(*res):
        assert (np.asarray(x) == np.asarray(y)).all()
    for X1 in (pkg.GraphCommStep(5, 3, 70, seed=3), pkg.GraphCommReLU(4, 4, 70, seed=3)):
        res = []
        for devices in (None, [0, 0]):
            with pkg.Engine(X1, 70, devices=devices) as eng:
                eng.seed(5)
                eng.init_spins_random()
                res.append(eng.standard_mc(0.8, 3000, 100) + (eng.get_config().s.copy(), eng.energy()))
        for x, y in zip(*res):
            assert (np.asarray(x) == np.asarray(y)).all()


def _lds_bytes_re(K1, K2, P, M):
    """re_rrr_lds_bytes + comm_lds_bytes of the RE LDS build (csrc/re_kernels.hpp, csrc/comm_kernels.hpp)"""
    Nk = K1 * K2
    N, W, PW = Nk * M, 2 * ((Nk * M + 63) // 64), (P + 63) // 64
    base = W * 4 + ((N * 2 + 3) & ~3) + ((N + 3) & ~3) + ((Nk + 3) & ~3) + 32 * 4 + 64 * 8 * 4
    return ((base + 7) & ~7) + M * PW * ((2 * K2 + 2) * 8 + (K2 + 1) * 64 * 2)


def test_largest_shapes(pkg):
    # GraphCommStepRE(25, 5, 2304, 5) takes 159 784 bytes of LDS (just under 160 KB) and runs in both builds; GraphCommStepRE(201, 5, 4096,
    # 5) does not fit and runs in the thread build without being asked to.  Tracked energy against a fresh one, debug checks on.
    assert _lds_bytes_re(25, 5, 2304, 5) <= 160 * 1024 < _lds_bytes_re(25, 5, 2368, 5)
    assert _lds_bytes_re(201, 5, 4096, 5) > 160 * 1024
    for X, envs in ((pkg.GraphCommStepRE(25, 5, 2304, 5, 1.0, 2.0), ({"RRRMC_RE_NO_LDS": "1"}, {"RRRMC_RE_LDS": "1"}, {})),
                    (pkg.GraphCommStepRE(201, 5, 4096, 5, 1.0, 2.0), ({},)),
                    (pkg.GraphCommReLULE(32, 4, 700, 5, 1.0, 2.0), ({"RRRMC_LE_NO_LDS": "1"}, {"RRRMC_LE_LDS": "1"}))):
        runs = []
        for env in envs:
            def run():
                with pkg.Engine(X, 2) as eng:
                    eng.set_debug_checks(True)
                    eng.seed(4)
                    eng.init_spins_random()
                    out = eng.rrr_mc(2.0, 2000, 1000) + eng.standard_mc(2.0, 2000, 1000)
                    Etr, E = eng.run_energy(), eng.energy()
                    assert (np.abs(Etr - E) <= 1e-10 * np.maximum(1.0, np.abs(E))).all()
                    return out + (eng.get_config().s.copy(),)
            runs.append(_with_env(env, run))
        for other in runs[1:]:
            for x, y in zip(runs[0], other):
                assert (np.asarray(x) == np.asarray(y)).all()


# ---- the stationary distribution ---------------------------------------------------------------------------------------------------
def _wilson_hilferty_limit(k):
    # the χ² quantile of the 1e-6 upper tail, Wilson-Hilferty (z = 4.7534 is the normal 1e-6 quantile)
    return k * (1 - 2 / (9 * k) + 4.753424 * (2 / (9 * k)) ** 0.5) ** 3


def _chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


def _state_index(Cfg, N):
    idx = np.zeros(Cfg.s.shape[0], np.int64)
    for j in range(N):                             # site 0 is the most significant bit, as itertools.product orders the states
        idx = idx * 2 + ((Cfg.s[:, 0] >> np.uint64(j)) & np.uint64(1)).astype(np.int64)
    return idx


# the instances: patterns fixed here, energies from the definition (comm_reference.energy_from_definition)
STEP_XI = [[1, 0, 1, 1, 0, 0, 1, 1, 0], [0, 0, 1, 1, 1, 0, 0, 1, 1]]           # CommStep(3, 3, P = 2): N = 9, 512 states
RELU_XI, RELU_Y = [[1, 0, 0, 1, 1, 1, 0, 1], [0, 1, 1, 0, 1, 0, 0, 1]], [1, 0]  # CommReLU(2, 4, P = 2): N = 8, 256 states
RE_XI = [[1, 0, 1], [0, 1, 1]]                                                  # RE(3, 3) over CommStep(1, 3, P = 2): N = 9, 512 states


@pytest.mark.parametrize("which", ["step", "relu"])
def test_standalone_final_configurations_follow_the_boltzmann_distribution(pkg, which):
    beta, R = 0.6, 65536
    if which == "step":
        K2, xi, y = 3, np.array(STEP_XI), None
        X = pkg.GraphCommStep.from_patterns(K2, xi)
    else:
        K2, xi, y = 4, np.array(RELU_XI), np.array(RELU_Y)
        X = pkg.GraphCommReLU.from_patterns(K2, xi, y)
    N = X.N
    states = list(itertools.product((0, 1), repeat=N))
    E = np.array([CR.energy_from_definition(K2, xi, y, s) for s in states], np.float64)
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    expected = p * R
    # every bin a valid χ² term; guaranteed by R e^{-β (Emax - Emin)} / 2^N >= 5 (here 65 536 e^{-1.2} / 2^N >= 38)
    assert R * np.exp(-beta * (E.max() - E.min())) / 2 ** N >= 5 and expected.min() >= 5
    with pkg.Engine(X, R) as eng:
        eng.seed(424242)
        eng.init_spins_random()
        eng.standard_mc(beta, 4000, 4000)
        idx = _state_index(eng.get_config(), N)
        assert (eng.run_energy() == E[idx]).all()
    stat = _chi2(np.bincount(idx, minlength=len(states)), expected)
    limit = _wilson_hilferty_limit(len(states) - 1)
    print("chi2 %s: %.1f (limit %.1f, smallest expected count %.1f)" % (which, stat, limit, expected.min()))
    assert stat < limit, (stat, limit)


@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_ensemble_final_configurations_follow_the_boltzmann_distribution(pkg, sampler):
    # GraphRobustEnsemble(3, 3, γ = 0.6, β = 1.2) over CommStep(K1 = 1, K2 = 3, P = 2): N = 9, 512 states; 65 536 chains, one final each
    Nk, M, gamma, beta_g, beta, R = 3, 3, 0.6, 1.2, 0.6, 65536
    xi = np.array(RE_XI)
    X1 = pkg.GraphCommStep.from_patterns(3, xi)
    X = pkg.GraphRobustEnsemble(Nk, M, gamma, beta_g, X1)
    N = X.N
    states = list(itertools.product((0, 1), repeat=N))

    def energy(s):                                 # -Σ_i log(2 cosh(γ μ_i)) / β + Σ_k E_k, E_k from the definition
        sg = 2 * np.asarray(s, np.int64).reshape(Nk, M) - 1
        E = -sum(np.log(2 * np.cosh(gamma * sg[i].sum())) / beta_g for i in range(Nk))
        return E + sum(CR.energy_from_definition(3, xi, None, (sg[:, k] + 1) // 2) for k in range(M))

    E = np.array([energy(s) for s in states])
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    expected = p * R
    assert expected.min() >= 5                     # every bin is a valid χ² term
    with pkg.Engine(X, R) as eng:
        eng.seed(424243)
        eng.init_spins_random()
        if sampler == "rrr":
            eng.rrr_mc(beta, 4000, 4000)
        else:
            eng.standard_mc(beta, 4000, 4000)
        idx = _state_index(eng.get_config(), N)
        assert np.abs(eng.run_energy() - E[idx]).max() < 1e-12
    stat = _chi2(np.bincount(idx, minlength=len(states)), expected)
    limit = _wilson_hilferty_limit(len(states) - 1)
    print("chi2 RE %s: %.1f (limit %.1f, smallest expected count %.1f)" % (sampler, stat, limit, expected.min()))
    assert stat < limit, (stat, limit)
