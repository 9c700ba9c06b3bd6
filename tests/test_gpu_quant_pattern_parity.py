"""GraphQuant over pattern-machine slices (GraphQPercStepT, GraphQPercLinearT, GraphQCommStepT, GraphQCommReLUT) on the device against the
Python restatement of the reference (tests/quant_pattern_reference.py): bit for bit.  The preconditions of every case — both branches of
rrrMC taken, accepts and rejects in each — are checked by tests/test_quant_pattern_cpu.py."""
import functools
import math

import numpy as np
import pytest

import boltzmann_law as BL
import quant_pattern_reference as QP
from re_reference import config_from_chunks

pytestmark = pytest.mark.gpu

R = 3
# the three kernel builds, forced by the existing switches, and what Engine.quant_pattern_build must report after a call: one thread per
# replica (0), one wavefront per replica with the slice state in HBM/L2 (1), one wavefront per replica with it staged in LDS (2)
BUILDS = {"thread": ({"RRRMC_QUANT_NO_WAVE": "1"}, 0), "wave-no-lds": ({"RRRMC_QUANT_NO_LDS": "1"}, 1), "lds": ({}, 2)}


@functools.lru_cache(maxsize=None)
def _reference(pkg, oracle, cid):
    """the reference's run of a case, both samplers, R replicas: computed once, shared, never modified"""
    case = QP.CASES[QP.CASE_IDS.index(cid)]
    X = QP.make_graph(pkg, case)
    beta = QP.BETA[case[1]]
    out = {"rrr": [], "std": []}
    for r in range(R):
        s = config_from_chunks(oracle.init_configs(QP.SEED, r, 1, X.N)[0], X.N)
        ref = QP.make_reference(X)
        run = QP.RrrRun(ref, s, beta, QP.SEED, oracle, replica=r, staged_thr=QP.STAGED_THR)
        Es = run.run(QP.ITERS, QP.STEP)
        out["rrr"].append((Es, s.copy(), run.accepted, run.staged_its) + run.cache_view() + (run.E, ref.renergies()))
        s = config_from_chunks(oracle.init_configs(QP.SEED, r, 1, X.N)[0], X.N)
        ref = QP.make_reference(X)
        Es, E, acc = QP.standard_mc(ref, s, beta, QP.ITERS, QP.STEP, QP.SEED, oracle, replica=r)
        out["std"].append((Es, s.copy(), acc, E, ref.renergies()))
    return X, out


def _bits(eng, X):
    return np.array([config_from_chunks(c, X.N) for c in eng.get_config().s])


def _observables_from_definition(X, s, Es_slices):
    """Qenergy, transverse_mag, overlaps of one configuration by the reference's formulas (QT.jl:113-122, 213-268), slice energies given"""
    M, Nk, N = X.M, X.Nk, X.N
    sl = s.reshape(M, Nk)
    e0 = -sum(int(((1 - 2 * sl[k]) * (1 - 2 * sl[k - 1])).sum()) for k in range(M))
    x = X.beta * X.fourK / 2
    tm = math.cosh(x) - (-e0 / N) * math.sinh(x)
    Q = -X.Gamma * tm
    for k in range(M):
        Q += Es_slices[k] / N
    ovs = [0.0] * (M // 2)
    for k1 in range(M - 1):
        for k2 in range(k1 + 1, M):
            d = min(k2 - k1, M + k1 - k2)
            ovs[d - 1] += Nk - 2 * int((sl[k1] ^ sl[k2]).sum())
    for d in range(1, (M - 1) // 2 + 1):
        ovs[d - 1] /= M * Nk
    if M % 2 == 0:
        ovs[M // 2 - 1] /= M * Nk / 2
    return Q, tm, ovs


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("cid", QP.CASE_IDS)
def test_both_samplers_bit_identical_to_the_reference(pkg, oracle, cid, build):
    """every shape through each of the three builds: all equal the reference, hence one another, bit for bit"""
    X, ref = _reference(pkg, oracle, cid)
    beta = QP.BETA[cid.split("-")[0]]
    env, want = BUILDS[build]
    with BL.with_env(env), pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(QP.SEED)
        eng.init_spins_random()
        E0 = eng.energy()
        Es, acc, st = eng.rrr_mc(beta, QP.ITERS, QP.STEP, staged_thr=QP.STAGED_THR)
        eng.sync()                                              # the debug mode reports here
        assert eng.quant_pattern_build() == want                # the kernel that ran is the one the case names
        pos, sizes = eng.rrr_cache()
        bits = _bits(eng, X)
        Etr = eng.run_energy()
        ren = eng.quant_renergies()
        Q, tm, ov = eng.quant_observables()
        for r in range(R):
            rEs, rs, racc, rst, rpos, rsizes, rE, rren = ref["rrr"][r]
            assert Es[r].tolist() == rEs and (bits[r] == rs).all() and (acc[r], st[r]) == (racc, rst)
            assert (pos[r] == rpos).all() and (sizes[r] == rsizes).all() and Etr[r] == rE
            assert ren[r].tolist() == [float(e) for e in rren]              # integers, or 2n / sqrt(Nk): one correctly rounded division
            dQ, dtm, dov = _observables_from_definition(X, rs, rren)
            assert ov[r].tolist() == dov                                     # integer sums and one division
            assert abs(tm[r] - dtm) <= 1e-12 * abs(dtm) and abs(Q[r] - dQ) <= 1e-12 * abs(dQ)      # libm's cosh / sinh enter
        # standardMC from the same start
        eng.seed(QP.SEED)
        eng.init_spins_random()
        assert (eng.energy() == E0).all()
        Es, acc = eng.standard_mc(beta, QP.ITERS, QP.STEP)
        assert eng.quant_pattern_build() == want
        bits = _bits(eng, X)
        Etr = eng.tracked_energy()
        ren = eng.quant_renergies()
        for r in range(R):
            rEs, rs, racc, rE, rren = ref["std"][r]
            assert Es[r].tolist() == rEs and (bits[r] == rs).all() and acc[r] == racc and Etr[r] == rE
            assert ren[r].tolist() == [float(e) for e in rren]


def test_module_level_observables_read_the_live_engine_and_a_given_configuration(pkg, oracle):
    X, ref = _reference(pkg, oracle, "cstep-3x3-3-65")
    with pkg.Engine(X, 1) as eng:
        eng.seed(QP.SEED)
        eng.init_spins_random()
        eng.rrr_mc(QP.BETA["cstep"], QP.ITERS, QP.STEP, staged_thr=QP.STAGED_THR)
        rs, rren = ref["rrr"][0][1], ref["rrr"][0][7]
        assert pkg.Renergies(X).tolist() == [float(e) for e in rren]
        dQ, dtm, dov = _observables_from_definition(X, rs, rren)
        assert pkg.overlaps(X).tolist() == dov and abs(pkg.Qenergy(X) - dQ) <= 1e-12 * abs(dQ) and abs(pkg.transverse_mag(X) - dtm) <= 1e-12 * abs(dtm)
        Cfg = eng.get_config()
    assert pkg.Renergies(X, Cfg).tolist() == [float(e) for e in rren]       # a context made for the call
    with pytest.raises(RuntimeError):
        pkg.Renergies(X)                                                    # no engine is running the graph any more


def test_build_rule_and_builds_continue_one_another(pkg):
    """RRRMC_QUANT_WAVE_MAX_R bounds the wave builds; a P of 4096 patterns (64 mask words) still stages; and a resumed run whose pieces go
    through the three builds in turn is the run made in one call by the thread build"""
    X = QP.make_graph(pkg, QP.CASES[QP.CASE_IDS.index("crelu-4x2-3-65")])
    beta, total, step = 1.5, 900, 50
    with BL.with_env({"RRRMC_QUANT_NO_WAVE": "1"}), pkg.Engine(X, R) as a:
        a.seed(31)
        a.init_spins_random()
        Ea, acca, sta = a.rrr_mc(beta, total, step, staged_thr=QP.STAGED_THR)
        Ca, pa = a.get_config().s.copy(), a.rrr_cache()
        assert a.quant_pattern_build() == 0
    with pkg.Engine(X, R) as b:
        b.set_debug_checks(True)
        b.seed(31)
        b.init_spins_random()
        b.set_resume(True)
        Es, acc, st, seen = [], np.zeros(R, np.int64), np.zeros(R, np.int64), []
        for n, env in ((217, {}), (301, {"RRRMC_QUANT_WAVE_MAX_R": str(R - 1)}), (149, {"RRRMC_QUANT_NO_LDS": "1"}), (233, {"RRRMC_QUANT_WAVE_MAX_R": str(R)})):
            with BL.with_env(env):
                e_, ac, s_ = b.rrr_mc(beta, n, step, staged_thr=QP.STAGED_THR)
            seen.append(b.quant_pattern_build())
            Es.append(e_)
            acc += ac
            st += s_
        assert seen == [2, 0, 1, 2]
        assert (Ea == np.concatenate(Es, axis=1)).all() and (acca == acc).all() and (sta == st).all()
        pb = b.rrr_cache()
        assert (Ca == b.get_config().s).all() and (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
    big = pkg.GraphQPercStepT(33, 4096, 3, QP.GAMMA, QP.BETA_GRAPH, seed=3)
    res = []
    for env, want in BUILDS.values():
        with BL.with_env(env), pkg.Engine(big, 2) as eng:
            eng.set_debug_checks(True)
            eng.seed(7)
            eng.init_spins_random()
            r1 = eng.rrr_mc(1.5, 300, 50)
            assert eng.quant_pattern_build() == want
            r2 = eng.standard_mc(1.5, 300, 50)
            res.append(r1 + r2 + (eng.get_config().s.copy(), eng.quant_renergies()))
    for other in res[1:]:
        for x, y in zip(res[0], other):
            assert (np.asarray(x) == np.asarray(y)).all()


def test_committee_with_one_hidden_unit_is_the_perceptron(pkg):
    P_ = pkg.GraphPercStep(33, 65, seed=9)
    C_ = pkg.GraphCommStep.from_patterns(1, P_.patterns())
    res = []
    for X in (pkg.GraphQPercStepT(P_, 3, QP.GAMMA, QP.BETA_GRAPH), pkg.GraphQCommStepT(C_, 3, QP.GAMMA, QP.BETA_GRAPH)):
        with pkg.Engine(X, R) as eng:
            eng.set_debug_checks(True)
            eng.seed(3)
            eng.init_spins_random()
            r1 = eng.rrr_mc(1.5, QP.ITERS, QP.STEP, staged_thr=QP.STAGED_THR)
            cache = eng.rrr_cache()
            r2 = eng.standard_mc(1.5, QP.ITERS, QP.STEP)
            res.append(r1 + cache + r2 + (eng.get_config().s.copy(), eng.quant_renergies()))
    for x, y in zip(*res):
        assert (np.asarray(x) == np.asarray(y)).all()


@pytest.mark.parametrize("cid", ["plin-33-3-65", "crelu-4x2-3-65"])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, cid):
    X = QP.make_graph(pkg, QP.CASES[QP.CASE_IDS.index(cid)])
    beta, total, step = QP.BETA[cid.split("-")[0]], 1500, 50
    rng = np.random.default_rng(12)
    cuts = sorted(set(rng.integers(1, total, 7).tolist()))
    pieces = np.diff([0] + cuts + [total]).tolist()
    with pkg.Engine(X, R) as a, pkg.Engine(X, R) as b:
        for e in (a, b):
            e.set_debug_checks(True)
            e.seed(31)
            e.init_spins_random()
        Ea, acca, sta = a.rrr_mc(beta, total, step, staged_thr=QP.STAGED_THR)
        b.set_resume(True)
        Es, acc, st = [], np.zeros(R, np.int64), np.zeros(R, np.int64)
        for n in pieces:
            e_, ac, s_ = b.rrr_mc(beta, n, step, staged_thr=QP.STAGED_THR)
            Es.append(e_)
            acc += ac
            st += s_
        assert (Ea == np.concatenate(Es, axis=1)).all() and (acca == acc).all() and (sta == st).all()
        assert (a.get_config().s == b.get_config().s).all()
        pa, pb = a.rrr_cache(), b.rrr_cache()
        assert (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
        assert (a.run_energy() == b.run_energy()).all()


@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hook_that_stops_one_replica_leaves_the_others_unchanged(pkg, sampler):
    X = QP.make_graph(pkg, QP.CASES[QP.CASE_IDS.index("cstep-3x3-3-65")])
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    beta, iters, step = 1.5, 1000, 100
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    seen = []

    def hook(it, X_, Cfg, acc, E):
        ren = pkg.Renergies(X_)                                  # read-only: does not disturb the run
        assert ren.shape == (R, X.M) and (ren >= 0).all()
        seen.append(it)
        return np.array([True, it < 3 * step, True])

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    for r in (0, 2):
        assert (np.asarray(Es0[r]) == np.asarray(Es1[r])).all() and (C0.s[r] == C1.s[r]).all()
    assert list(Es1[1]) == list(Es0[1][:3])                      # the stopped replica: its samples up to its stop


def test_two_shard_context_equals_single(pkg):
    X = QP.make_graph(pkg, QP.CASES[QP.CASE_IDS.index("crelu-4x2-3-65")])
    res = []
    for devices in (None, [0, 0]):
        with pkg.Engine(X, 64, devices=devices) as eng:
            eng.set_debug_checks(True)
            eng.seed(5)
            eng.init_spins_random()
            r1 = eng.rrr_mc(1.5, QP.ITERS, QP.STEP, staged_thr=QP.STAGED_THR)
            cache = eng.rrr_cache()
            r2 = eng.standard_mc(1.5, QP.ITERS, QP.STEP)
            res.append(r1 + cache + r2 + (eng.get_config().s.copy(), eng.energy(), eng.quant_renergies()) + eng.quant_observables())
    for x, y in zip(*res):
        assert (np.asarray(x) == np.asarray(y)).all()


def test_refusals_and_argument_checks(pkg):
    import ctypes as C
    L = pkg.lib()
    X = QP.make_graph(pkg, QP.CASES[QP.CASE_IDS.index("pstep-min-3-3-1")])
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call in (lambda: eng.bkl_mc(1.0, 10, 1), lambda: eng.wtm_mc(1.0, 2, 1.0), lambda: eng.extremal_opt(1.2, 10, 1)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3                             # RRRMC_ERR_UNSUPPORTED
        eng.rrr_mc(1.0, 10, 1)                                   # and the context is still good

    def create(kind, Nk, K2, M):
        ctx = C.c_void_p()
        rc = L.rrrmc_ctx_create_quant_pattern(C.byref(ctx), kind, Nk, K2, M, 2, 0, 0)
        if ctx:
            L.rrrmc_ctx_destroy(ctx)
        return rc

    assert create(3, 33, 0, 3) == 0 and create(5, 9, 3, 3) == 0 and create(6, 8, 2, 3) == 0
    assert create(3, 32, 0, 3) == 1 and create(4, 32, 0, 3) == 1         # Nk even: RRRMC_ERR_INVALID_ARG
    assert create(5, 12, 3, 3) == 1 and create(5, 15, 5, 3) == 0 and create(5, 10, 5, 3) == 1      # K1 / K2 even (step)
    assert create(6, 9, 3, 3) == 1 and create(6, 6, 2, 3) == 1           # K1 / K2 odd (ReLU)
    assert create(5, 10, 3, 3) == 1                                      # Nk not a multiple of K2
    assert create(3, 33, 0, 2) == 1                                      # M > 2 (QT.jl:47)
    assert create(2, 33, 0, 3) == 1                                      # not a pattern slice kind
    assert create(3, 32769, 0, 3) == 3 and create(3, 21847, 0, 3) == 3   # Nk <= 32767, N = Nk M <= 65535: RRRMC_ERR_UNSUPPORTED
    assert create(5, 32769, 1, 3) == 3 and create(5, 21847, 1, 3) == 3 and create(6, 21848, 2, 3) == 3      # the committee kinds alike
    # everything is refused until rrrmc_quant_set_field has been called
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create_quant_pattern(C.byref(ctx), 3, 33, 0, 3, 2, 0, 0) == 0
    try:
        xi = pkg.GraphPercStep(33, 5, seed=1).xi
        assert L.rrrmc_set_patterns(ctx, xi.reshape(-1), 5) == 0
        assert L.rrrmc_set_patterns(ctx, xi.reshape(-1), 4097) == 3      # 1 <= P <= 4096
        assert L.rrrmc_set_comm_patterns(ctx, 1, xi.reshape(-1), None, 5) == 2      # the perceptron setter is this context's
        assert L.rrrmc_seed(ctx, 1) == 0 and L.rrrmc_init_spins_random(ctx) == 0
        E = np.zeros(2)
        assert L.rrrmc_energy_f64(ctx, E) == 2 and L.rrrmc_standard_mc_async(ctx, 1.0, 10, 1) == 2
        assert L.rrrmc_rrr_mc_async(ctx, 1.0, 1.0, 10, 1, 0.5, 5.0) == 2 and L.rrrmc_quant_renergies(ctx, np.zeros(6)) == 2
        assert L.rrrmc_quant_observables(ctx, 1.0, 0.5, None, None, None) == 2
        assert L.rrrmc_quant_set_field(ctx, 1.0, 1.0) == 0 and L.rrrmc_energy_f64(ctx, E) == 0
    finally:
        L.rrrmc_ctx_destroy(ctx)
