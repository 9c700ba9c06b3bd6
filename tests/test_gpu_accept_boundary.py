"""Every accept decision ``x >= 0 || rand() < exp(x)`` (src/RRRMC.jl:39) where the kernels could differ from the oracle without a random run
noticing: on the last bits of det_exp (the probes of tests/accept_boundary.py: the in-band branch of the three filter kernels decides the
move), at large |x| (forced exponential, subnormal and zero results, an estimate that underflows, x = -inf), and at the edges of beta (negative,
signed zero, beyond every exponent, infinite).  Everything bit for bit against the oracle; a (family, beta) the library does not compute
must be refused with a message that names beta."""
import math

import numpy as np
import pytest

import accept_boundary as AB

pytestmark = pytest.mark.gpu

SK_ENV = ("RRRMC_SK_RB", "RRRMC_SK_LEGACY", "RRRMC_SK_BLOCK_V1", "RRRMC_SK_THREADS")
SPF_ENV = ("RRRMC_SPF_TEAM", "RRRMC_SPF_TEAM_WAVES", "RRRMC_SPF_TEAM_WIDTH")
LEGACY = {"RRRMC_SK_LEGACY": "1"}
SPF_BUILDS = ({"RRRMC_SPF_TEAM_WIDTH": "64"}, {"RRRMC_SPF_TEAM_WIDTH": "32"}, {"RRRMC_SPF_TEAM_WIDTH": "16"}, {"RRRMC_SPF_TEAM": "0"})


def _sk_builds(N):
    """the default (sk_hblock_kernel; split below N = 512), whole-group and split builds of both blocked kernels where a split build exists
    (N <= 1024), sk_block_kernel alone beyond, and the one-attempt-at-a-time kernel"""
    if N <= 1024:
        return ({}, {"RRRMC_SK_RB": "8"}, {"RRRMC_SK_RB": "4"}, {"RRRMC_SK_BLOCK_V1": "1", "RRRMC_SK_RB": "8"},
                {"RRRMC_SK_BLOCK_V1": "1", "RRRMC_SK_RB": "4"}, LEGACY)
    return ({}, {"RRRMC_SK_BLOCK_V1": "1"}, LEGACY)


def _set_env(monkeypatch, names, env):
    for k in names:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _graph(pkg, O, key):
    p = AB.path(O, key)
    kind, N = key
    if kind == "skn":
        X = pkg.GraphSKNormal(N, seed=AB.GSEED + N)
    elif kind == "skb":
        X = pkg.GraphSK(N, seed=AB.GSEED + N)
    elif kind == "rrgn":
        X = pkg.GraphRRGNormal(96, 3, seed=AB.GSEED)
    elif kind == "ean":
        X = pkg.GraphEANormal(2, 4, seed=AB.GSEED)
    else:
        L, D, M, Gamma, beta_g = AB.QEAT
        X1 = pkg.GraphEANormal(L, D, seed=AB.GSEED)
        assert (X1.A == p.A).all() and (X1.J == p.J).all()
        X = pkg.GraphQEAT(X1, M, Gamma, beta_g)                       # GraphQEAT(X::GraphEANormal, M, Γ, β): QAliases.jl:77-83
        assert X.fourK == p.fourK and X.N == p.N
        return X, p
    assert (X.J == p.J).all() and (kind[0] == "s" or (X.A == p.A).all())          # the oracle's graph is the library's
    return X, p


def _device(eng, seed, beta, iters, fields):
    eng.seed(seed)
    eng.init_spins_random()
    Es, acc = eng.standard_mc(beta, iters, 1)
    return Es, eng.get_config().s.copy(), acc, (eng.fields() if fields else None)


def _assert_same(dev, ref, what):
    for name, d, r in zip(("Es", "config", "accepted", "fields"), dev, ref):
        if r is not None:
            assert d.shape == r.shape and (d == r).all(), "%s differs from the oracle: %s" % (name, what)


def _check_spf_build(eng, env):
    nw, tw, slots = eng.spf_team_build()
    if env.get("RRRMC_SPF_TEAM") == "0":
        assert (nw, tw, slots) == (0, 0, 0)
    else:
        assert tw == int(env["RRRMC_SPF_TEAM_WIDTH"]) and nw in (8, 16) and slots > 0


def _probe_case(pkg, O, monkeypatch, key, t, builds, env_names, check_build=None):
    X, p = _graph(pkg, O, key)
    R, iters = AB.PATHS[key], AB.iters_for(t)
    tg = AB.targets(O, key, t)
    assert len(tg) >= 3, "fewer than 3 live targets for %r, attempt %d" % (key, t)
    refs = {(q.seed, b): p.ref(q.seed, b, iters, R) for q in tg for b in AB.four_betas(q)}
    for q in tg:
        assert refs[(q.seed, q.beta_acc)][2][q.r] != refs[(q.seed, q.beta_rej)][2][q.r]          # the probe is live
    fields = refs[(tg[0].seed, tg[0].beta_acc)][3] is not None
    with pkg.Engine(X, R) as eng:
        for env in builds:
            if env is LEGACY and t not in (1, 65):
                continue                                            # one attempt at a time: the lane within the block means nothing to it
            _set_env(monkeypatch, env_names, env)
            if check_build:
                check_build(eng, env)
            for q in tg:
                got = {}
                for b in AB.four_betas(q):
                    got[b] = _device(eng, q.seed, b, iters, fields)
                    _assert_same(got[b], refs[(q.seed, b)], "%r build %r seed %d replica %d attempt %d beta %r" % (key, env, q.seed, q.r, t, b))
                assert got[q.beta_acc][2][q.r] != got[q.beta_rej][2][q.r]


@pytest.mark.parametrize("t", AB.CLASSES)
@pytest.mark.parametrize("key", [k for k in AB.PATHS if k[0] in ("skn", "skb")], ids=lambda k: "%s%d" % k)
def test_dense_sk_decides_like_det_exp_on_its_last_bits(pkg, oracle, monkeypatch, key, t):
    """sk_hblock_kernel (Float32 log filter, the constants of det_exp rebuilt inside the band) and sk_block_kernel (Float64 log filter, a
    band entered once in 10^9 random evaluations): a move whose verdict changes between two adjacent betas, in every lane class, every build."""
    _probe_case(pkg, oracle, monkeypatch, key, t, _sk_builds(key[1]), SK_ENV)


@pytest.mark.parametrize("t", AB.CLASSES)
@pytest.mark.parametrize("key", [("rrgn", 96), ("ean", 16)], ids=lambda k: "%s%d" % k)
def test_spf_team_decides_like_det_exp_on_its_last_bits(pkg, oracle, monkeypatch, key, t):
    """spf_team_kernel's v_exp_f32 filter, both copies: whole groups (width 64), the fused pairs of teams of 32 and 16 replicas (K = 3, and
    K = 8 in eight-wavefront teams), and spf_sweep_kernel, which has no filter; 70 replicas leave the last team partly filled."""
    _probe_case(pkg, oracle, monkeypatch, key, t, SPF_BUILDS, SPF_ENV, _check_spf_build)


@pytest.mark.parametrize("t", AB.classes_of(("qeat", 128)))
def test_control_without_a_filter(pkg, oracle, monkeypatch, t):
    """GraphQEAT's standardMC calls det_exp for every move with x < 0: the probes themselves are sound where no filter is in the way"""
    _probe_case(pkg, oracle, monkeypatch, ("qeat", 128), t, ({},), ())


@pytest.mark.parametrize("key", AB.LARGE_X_PATHS, ids=lambda k: "%s%d" % k)
def test_large_negative_x(pkg, oracle, monkeypatch, key):
    """x = -90 and -110 (the Float32 estimate of spf_team_kernel is denormal, then zero), -699 / -701 (both sides of the forced exponential of
    the SK block kernels), -722.6 (subnormal ldexp result), -745.1 / -745.3 (both sides of det_exp's cut to zero), then beta = 1e5, 1e300, inf
    (x beyond every exponent; -inf, and NaN wherever a field is zero): 256 iterations of every build against the oracle."""
    X, p = _graph(pkg, oracle, key)
    R, iters = AB.PATHS[key], 256
    seed, r, lane, site, rows = AB.large_x_case(oracle, key)
    for x, beta, xa in rows[:len(AB.LARGE_X)]:
        assert abs(xa - x) < 1e-9                                    # the start block really has a lane there (checked in full on the CPU side)
    sk = key[0] in ("skn", "skb")
    refs = {beta: p.ref(seed, beta, iters, R) for _, beta, _ in rows}
    with pkg.Engine(X, R) as eng:
        for env in (_sk_builds(key[1]) if sk else SPF_BUILDS):
            _set_env(monkeypatch, SK_ENV if sk else SPF_ENV, env)
            if not sk:
                _check_spf_build(eng, env)
            for x, beta, xa in rows:
                _assert_same(_device(eng, seed, beta, iters, True), refs[beta], "%r build %r seed %d beta %r (x = %r in lane %d)" % (key, env, seed, beta, xa, lane))


# ---- the sign and the infiniteness of beta -----------------------------------------------------------------------------------------------
BETAS = (-0.4, -0.0, 0.0, 1e300, math.inf, -math.inf)
SEED, R33, ITERS, STEP = 20251, 33, 2000, 100


def _c_oracle(fn, conv=lambda e: e):
    """reference of the families the C oracle covers: every replica"""
    def ref(beta, C0):
        out = [fn(beta, C0[r], r) for r in range(len(C0))]
        return np.stack([conv(o[0]) for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64)
    return ref, None


def _py_reference(O, mod, make, N):
    """reference of the families restated in Python (tests/*_reference.py): the two ends of the replica range"""
    import re_reference as RE

    def ref(beta, C0):
        rows = []
        for r in (0, len(C0) - 1):
            s = RE.config_from_chunks(C0[r], N)
            es, E, a = mod.standard_mc(make(), s, beta, ITERS, STEP, SEED, O, replica=r)
            rows.append((np.array(es, np.float64), RE.chunks_from_config(s), a))
        return np.stack([o[0] for o in rows]), np.stack([o[1] for o in rows]), np.array([o[2] for o in rows], np.int64)
    return ref, (0, R33 - 1)


def _family(pkg, O, name):
    """-> (X, env, ref(beta, C0) -> (Es, configs, accepted), replicas checked or None = all, run(eng, beta) or None = standard_mc)"""
    sp = lambda X, form: _c_oracle(lambda b, c, r: O.standard_mc_sparse(X.A, X.J.astype(np.int32), b, ITERS, STEP, SEED, c, replica=r, form=form))
    if name in ("rrg128k3", "rrg128k3_generic", "rrg128k3_big"):
        X = pkg.GraphRRG(128, 3, seed=SEED)
        env = {"rrg128k3_generic": {"RRRMC_SWEEP_GENERIC": "1"}, "rrg128k3_big": {"RRRMC_FORCE_BIG": "1"}}.get(name, {})
        return (X, env) + sp(X, "rrg") + (None,)
    if name == "ea4x2":
        X = pkg.GraphEA(4, 2, seed=SEED)                                                    # K = 4: a class with dE = 0
        return (X, {}) + sp(X, "ea") + (None,)
    if name == "rrg128k3_colored":
        X = pkg.GraphRRG(128, 3, seed=SEED)
        color, A, J, sweeps = O.greedy_coloring(X.A), X.A, X.J.astype(np.int32), 16

        def run(eng, beta):
            eng.set_coloring(color)
            eng.colored_count_accepted(True)
            eng.colored_sweeps_async(beta, sweeps, 1)
            eng.sync()
            return eng.fetch_results()
        ref, _ = _c_oracle(lambda b, c, r: O.colored_sweeps_sparse(A, J, color, b, sweeps, 1, SEED, c, replica=r))
        return X, {}, ref, None, run
    if name in ("ea4x4_k8", "rrg10_levels"):
        lev = (-1, 1) if name == "ea4x4_k8" else (-1, 0, 1)
        X = pkg.GraphEA(4, 4, lev, seed=SEED) if name == "ea4x4_k8" else pkg.GraphRRG(10, 3, lev, seed=SEED)
        form = "ea" if name == "ea4x4_k8" else "rrg"
        units, mul, div = pkg.level_units(lev)
        assert X.model_kind == 7
        return (X, {}) + _c_oracle(lambda b, c, r: O.standard_mc_lev(X.A, X.J, b, ITERS, STEP, SEED, c, replica=r, form=form, mul=mul, div=div),
                                   X.energy_value) + (None,)
    if name == "rrg10_discretized":
        lev = (-1, 0, 1)
        X = pkg.GraphRRGNormalDiscretized(10, 3, lev, seed=SEED)
        _, mul, div = O.dfloat_units(lev)
        return (X, {}) + _c_oracle(lambda b, c, r: O.standard_mc_dbl(X.A, X.dJ, X.rJ, b, ITERS, STEP, SEED, c, replica=r, form="rrg", mul=mul, div=div)) + (None,)
    if name in ("skn37", "skb37", "rrgn96"):
        key = {"skn37": ("skn", 37), "skb37": ("skb", 37), "rrgn96": ("rrgn", 96)}[name]
        X, p = _graph(pkg, O, key)
        chain = lambda b, c, r: p.chain(b, ITERS, SEED, c, r)
        step = lambda o: (o[0][STEP - 1::STEP],) + tuple(o[1:3])                            # (the paths sample every iteration)
        return (X, {}) + _c_oracle(lambda b, c, r: step(chain(b, c, r))) + (None,)
    if name == "quant_rrg":
        X1 = pkg.GraphRRG(10, 3, seed=SEED)
        X = pkg.GraphQuant(X1, 8, 0.5, 2.0)
        A, J = X1.A, X1.J.astype(np.int32)
        return (X, {}) + _c_oracle(lambda b, c, r: O.standard_mc_quant(A, J, 8, X.fourK, b, ITERS, STEP, SEED, c, replica=r)) + (None,)
    if name == "perc_step":
        import perc_reference as PR
        X = pkg.GraphPercStep(33, 70, seed=SEED)
        xi = X.patterns()
        return (X, {}) + _py_reference(O, PR, lambda: PR.make(xi, False), X.N) + (None,)
    if name == "comm_step":
        import comm_reference as CR
        X = pkg.GraphCommStep(3, 3, 20, seed=SEED)
        xi, y = X.patterns(), X.labels()
        return (X, {}) + _py_reference(O, CR, lambda: CR.make(3, xi, y), X.N) + (None,)
    if name == "sat":
        import sat_reference as SR
        X = pkg.GraphSAT(10, 3, 4.2, seed=SEED)
        return (X, {}) + _py_reference(O, SR, lambda: SR.ClauseCache(X.N, X.A, X.J), X.N) + (None,)
    raise KeyError(name)


FAMILIES = ("rrg128k3", "rrg128k3_generic", "rrg128k3_big", "rrg128k3_colored", "ea4x2", "ea4x4_k8", "rrg10_levels", "rrg10_discretized", "skn37", "skb37",
            "rrgn96", "perc_step", "comm_step", "sat", "quant_rrg")
# The +-J kernels accept every move with dE <= 0 in their code: right for finite beta >= 0, and for an infinite beta where no move has dE = 0
# (odd degree).  Elsewhere the entry points refuse (README, "Limits"); every other family computes the general rule at every beta.
PM1_ODD, PM1_EVEN = ("rrg128k3", "rrg128k3_generic", "rrg128k3_big", "rrg128k3_colored"), ("ea4x2",)
REFUSED = {(f, b) for f in PM1_ODD + PM1_EVEN for b in (-0.4, -math.inf)} | {(f, math.inf) for f in PM1_EVEN}


@pytest.mark.parametrize("beta", BETAS, ids=repr)
@pytest.mark.parametrize("family", FAMILIES)
def test_sign_and_infinity_of_beta(pkg, oracle, monkeypatch, family, beta):
    """The reference's standardMC takes any beta (only rrrMC asks for a finite one, RRRMC.jl:159,230): beta < 0 accepts every move with
    dE > 0 and a move with dE < 0 with probability exp(-beta dE); an infinite beta makes x = -beta dE = NaN where dE = 0, which is
    rejected.  Every family either computes exactly that or refuses the call, naming beta — never another chain."""
    for k in ("RRRMC_SWEEP_GENERIC", "RRRMC_FORCE_BIG"):
        monkeypatch.delenv(k, raising=False)
    X, env, ref, reps, run = _family(pkg, oracle, family)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pkg.Engine(X, R33) as eng:
        eng.seed(SEED)
        eng.init_spins_random()
        C0 = eng.get_config().s.copy()
        assert (C0 == oracle.init_configs(SEED, 0, R33, X.N)).all()
        try:
            Es, acc = run(eng, beta) if run else eng.standard_mc(beta, ITERS, STEP)
        except pkg.RRRMCError as e:
            assert (family, beta) in REFUSED, "refused a beta the library is expected to compute: %s" % e
            assert e.code in (1, 3) and "beta" in str(e)               # RRRMC_ERR_INVALID_ARG / RRRMC_ERR_UNSUPPORTED
            assert (eng.get_config().s == C0).all()                    # a refused call changes nothing
            return
        assert (family, beta) not in REFUSED, "expected a refusal"
        C1 = eng.get_config().s.copy()
        if family in ("rrg128k3", "rrg128k3_generic", "rrg128k3_big", "ea4x2"):       # which +-J kernel ran: the big-N ones, the generic sweep, a sweep build
            b = eng.sweep_build()
            assert b == -1 if family == "rrg128k3_big" else b == 0 if family == "rrg128k3_generic" else b >= 0
    rEs, rC, racc = ref(beta, C0)
    sel = slice(None) if reps is None else list(reps)
    assert (np.asarray(Es)[sel] == rEs).all() and (C1[sel] == rC).all(), "%s at beta = %r is another chain than the reference's" % (family, beta)
    assert (np.asarray(acc)[sel] == racc).all()
    if beta == 0.0:                                                    # x = -beta dE is a zero of either sign: x >= 0, every move accepted
        assert (np.asarray(acc) == (16 * X.N if run else ITERS)).all()
