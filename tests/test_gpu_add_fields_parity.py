"""GPU parity for GraphAddFields / GraphAddSubFields (src/graphs/AddFields.jl): rrrMC and standardMC equal the plain-Python restatement
(tests/add_fields_reference.py) bit for bit — spins, sampled energies, accepted and staged counts, and the DeltaECacheCont that
``rrrmc_af_cache`` returns — through the LDS build and the forced global-memory build, with ``rrrmc_af_build`` showing which ran, and with
the debug checks on in every run.  Cut, resumed and two-shard runs equal the run made in one call; standardMC on the wrappers equals the
stand-alone engines of g; what is not wired answers RRRMC_ERR_UNSUPPORTED."""
import os

import numpy as np
import pytest

import add_fields_reference as AF
import re_reference as RE
import sat_reference as SR

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 1, 2
SEED = 90417
BETA_UNDERFLOW = 40.0          # 2 |h| β = 800 for the fields of ±10 below: exp(-800) is exactly 0; the other weights stay positive


class _env:
    def __init__(self, build):
        self.build = build

    def __enter__(self):
        self.old = os.environ.pop("RRRMC_AF_NO_LDS", None)
        if self.build == GLOBAL:
            os.environ["RRRMC_AF_NO_LDS"] = "1"

    def __exit__(self, *a):
        os.environ.pop("RRRMC_AF_NO_LDS", None)
        if self.old is not None:
            os.environ["RRRMC_AF_NO_LDS"] = self.old


def fields(N, seed=5):
    """Gaussian fields with exact zeros of both signs and, where there is room, two fields of ±10"""
    h = np.random.default_rng(seed).normal(size=N)
    h[0] = 0.0
    if N > 4:
        h[N // 2] = -0.0
        h[1], h[N - 2] = 10.0, -10.0
    return h


def graph(pkg, name):
    if name == "sat33":
        return pkg.GraphSAT(33, 3, 4.2, seed=1033)
    if name == "ragged":
        return pkg.GraphSAT.from_clauses(*SR.ragged_instance())
    if name == "perc":
        return pkg.GraphPercStep(21, 12, seed=3)
    if name == "perclin":
        return pkg.GraphPercLinear(21, 12, seed=3)
    if name == "sk":
        return pkg.GraphSK(20, seed=4)
    if name == "skn":
        return pkg.GraphSKNormal(20, seed=4)
    if name == "commstep":
        return pkg.GraphCommStep(3, 7, 10, seed=6)
    if name == "commrelu":
        return pkg.GraphCommReLU(4, 6, 10, seed=6)
    if name == "commqu":
        return pkg.GraphCommQu(4, 6, 10, seed=6)
    if name.startswith("empty"):
        return None
    if name.startswith("sat"):
        N = int(name[3:])
        return pkg.GraphSAT(N, min(3, N), 2.0, seed=2000 + N)
    raise KeyError(name)


def wrap(pkg, sub, name):
    g = graph(pkg, name)
    N = g.N if g is not None else int(name[5:])
    return (pkg.GraphAddSubFields if sub else pkg.GraphAddFields)(fields(N), g)


def run_rrr(pkg, X, R, beta, thr, build, pieces, step, devices=None, C0=None):
    """an rrrMC run made of the given pieces (resumed calls), from random spins or from C0: what the engine hands back"""
    with _env(build), pkg.Engine(X, R, devices=devices) as eng:
        eng.set_debug_checks(True)
        eng.seed(SEED)
        if C0 is None:
            eng.init_spins_random()
        else:
            eng.set_config(C0)
        assert eng.af_build() == 0
        C0 = eng.get_config()
        E0 = np.atleast_1d(eng.energy())
        Es, acc, st = [], np.zeros(R, np.int64), np.zeros(R, np.int64)
        for k, n in enumerate(pieces):
            eng.set_resume(k > 0)
            e, a, s = eng.rrr_mc(beta, n, step, staged_thr=thr)
            Es.append(np.atleast_2d(e))
            acc += a
            st += s
            assert eng.af_build() == build
        eng.set_resume(False)
        return dict(C0=C0, E0=E0, Es=np.concatenate(Es, axis=1), acc=acc, staged=st, C1=eng.get_config(), Etr=np.atleast_1d(eng.run_energy()),
                    cache=eng.af_cache())


def check_rrr(oracle, X, out, R, beta, thr, iters, step, replicas=None):
    N = X.N
    for r in sorted((replicas or {0, R - 1}) & set(range(R))):
        s = RE.config_from_chunks(out["C0"].s[r], N)
        Xr = AF.reference_of(X)
        run = AF.AfRun(Xr, s, beta, SEED, oracle, replica=r, staged_thr=thr)
        assert out["E0"][r] == run.E, r
        es = run.run(iters, step)
        assert out["Es"][r].tolist() == es, r
        assert out["acc"][r] == run.accepted and out["staged"][r] == run.staged_its, r
        assert (out["C1"].s[r] == RE.chunks_from_config(s)).all(), r
        assert out["Etr"][r] == run.E, r
        dEs, v, z, tref = run.cache_view()
        assert out["cache"][0][r].tolist() == dEs and out["cache"][1][r].tolist() == v, r
        assert out["cache"][2][r] == z and out["cache"][3][r] == tref, r
        assert all(v[i] == run.prior(beta * dEs[i]) for i in range(N))
    return run


# ---- the full matrix --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 33])
@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("beta", [0.0, 1.0, BETA_UNDERFLOW])
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.5], ids=["direct", "default", "staged"])
@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
@pytest.mark.parametrize("name", ["sat33", "ragged", "perc"])
def test_rrr_mc_bit_exact(pkg, oracle, name, sub, thr, beta, build, R):
    iters, step = 600, 50          # max(N, 100)-spaced refreshes fall inside the run (the direct branch makes up to two setindex! per iteration)
    X = wrap(pkg, sub, name)
    out = run_rrr(pkg, X, R, beta, thr, build, [iters], step)
    assert out["Es"].shape == (R, iters // step) and out["Es"].dtype == np.float64
    run = check_rrr(oracle, X, out, R, beta, thr, iters, step)
    if beta <= 1.0:          # (at the underflow β a chain may freeze before max(N, 100) calls of setindex!)
        assert run.ds.refreshes >= 1
    if thr == 0.0:
        assert run.staged_its == 0
    if thr == 1.5:
        assert run.staged_its == iters


# ---- getel's own refresh ----------------------------------------------------------------------------------------------------------------
# With the graphs of the matrix above the `k >= N || v[k+1] == 0` test of getel is evaluated at every draw and is never true: spins that g
# holds against their field keep a weight of 1, and z stays exact.  It becomes true without a loss of precision when ALL weights are at the
# rounding scale of the z they were subtracted from: fields of 0.4 .. 0.55 give weights exp(-32) .. exp(-44) at β = 40, a field of -10 on the last
# spin gives an exact 0 where an overshooting draw lands, and g leaves most spins free.  The start configurations are picked with the
# restatement: a few spins against their field, a chain that refreshes inside getel, none that meets the reference's precision-loss error.
def underflow_fields(N):
    rng = np.random.default_rng(5)
    h = rng.uniform(0.4, 0.55, size=N) * rng.choice([-1.0, 1.0], size=N)
    h[N - 1] = -10.0
    return h


def _underflow_graph(pkg, kind, sub):
    g = None if kind == "empty33" else pkg.GraphSAT(33, 3, 0.5, seed=7)
    return (pkg.GraphAddSubFields if sub else pkg.GraphAddFields)(underflow_fields(33), g)


_STARTS = {}


def pick_start(pkg, oracle, kind, sub, thr, R=8, iters=600):
    """(C0, getel-triggered refreshes of every chain): the first of 40 candidate batches in which some chain refreshes inside getel"""
    key = (kind, sub, thr)
    if key not in _STARTS:
        X = _underflow_graph(pkg, kind, sub)
        aligned = (X.fields < 0).astype(np.int64)                                  # σ_i = -sign(h_i): every ΔE0 > 0
        for cand in range(40):
            rng = np.random.default_rng(1000 + cand)
            S = [aligned ^ (rng.random(X.N) < 0.1).astype(np.int64) for _ in range(R)]
            counts = []
            try:
                for r in range(R):
                    run = AF.AfRun(AF.reference_of(X), S[r].copy(), BETA_UNDERFLOW, SEED, oracle, replica=r, staged_thr=thr)
                    run.run(iters, 50)
                    counts.append(run.ds.getel_refreshes)
            except AF.PrecisionLoss:
                continue
            if sum(counts) >= 1:
                C0 = pkg.Config(X.N, R)
                for r in range(R):
                    C0.s[r] = RE.chunks_from_config(S[r])
                _STARTS[key] = (C0, counts)
                break
        else:
            raise AssertionError("no candidate start refreshes inside getel: %r" % (key,))
    return _STARTS[key]


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.5], ids=["direct", "default", "staged"])
@pytest.mark.parametrize("kind", ["empty33", "sat33-sparse"])
def test_getel_refreshes_on_a_zero_weight_and_descends_again(pkg, oracle, kind, thr, build):
    # GraphAddFields only: a GraphAddSubFields chain samples g's own law, which does not favour the fields, so spins keep turning against
    # them and weights of 1 keep z exact (no refresh inside getel in 360 chains of the restatement); getel is the same code for both
    R, iters, step, sub = 8, 600, 50, 0
    X = _underflow_graph(pkg, kind, sub)
    p = sorted(oracle.det_exp(-BETA_UNDERFLOW * abs(2 * x)) for x in X.fields)
    assert p[0] == 0.0 and 0.0 < p[1] and p[-1] < 2.0 ** -46                       # one exact 0; every other weight below the rounding of 1 + w
    C0, counts = pick_start(pkg, oracle, kind, sub, thr)
    out = run_rrr(pkg, X, R, BETA_UNDERFLOW, thr, build, [iters], step, C0=C0)
    total = 0
    for r in range(R):
        run = check_rrr(oracle, X, out, R, BETA_UNDERFLOW, thr, iters, step, replicas={r})
        assert run.ds.getel_refreshes == counts[r]
        total += run.ds.getel_refreshes
    assert total >= 1


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
def test_the_loss_of_precision_is_reported(pkg, oracle, build):
    """every weight exactly 0 from the start: getel lands on an empty element with nothing to refresh (DynamicSamplers.jl:147)"""
    N, R = 5, 3
    h = np.array([10.0, -10.0, 10.0, 10.0, -10.0])
    X = pkg.GraphAddFields(h, None)
    s = (h < 0).astype(np.int64)
    with pytest.raises(AF.PrecisionLoss):
        AF.AfRun(AF.reference_of(X), s.copy(), BETA_UNDERFLOW, SEED, oracle).run(10, 1)
    C0 = pkg.Config(N, R)
    for r in range(R):
        C0.s[r] = RE.chunks_from_config(s)
    with _env(build), pkg.Engine(X, R) as eng:
        eng.seed(SEED)
        eng.set_config(C0)
        with pytest.raises(pkg.RRRMCError) as e:
            eng.rrr_mc(BETA_UNDERFLOW, 10, 1)
        assert e.value.code == 2 and "Unrecoverable loss of precision" in str(e.value) and "(of 3)" in str(e.value)
        for r in range(R):
            C0.s[r] = RE.chunks_from_config(1 - s)
        eng.set_config(C0)                                                         # the context is usable again (at β = 1 no weight is 0)
        Es, acc, _ = eng.rrr_mc(1.0, 10, 1)
        assert Es.shape == (R, 10) and (acc > 0).all()


# ---- tree shapes: levs = 0, 1, 2; N2 = N; one level past a six-level round trip with 63 padded leaves -------------------------------------
@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("N", [1, 2, 3, 64, 65])
@pytest.mark.parametrize("kind", ["empty", "sat"])
def test_tree_shapes(pkg, oracle, kind, N, build):
    for sub in (0, 1):
        X = wrap(pkg, sub, "%s%d" % (kind, N))
        assert X.N == N
        out = run_rrr(pkg, X, 3, 0.7, 0.5, build, [400], 40)
        check_rrr(oracle, X, out, 3, 0.7, 0.5, 400, 40, replicas={0, 1, 2})


# ---- the other kinds of g ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
@pytest.mark.parametrize("name", ["sk", "skn", "perclin", "commstep", "commrelu", "commqu"])
def test_other_kinds_bit_exact(pkg, oracle, name, sub, build):
    X = wrap(pkg, sub, name)
    out = run_rrr(pkg, X, 5, 1.0, 0.5, build, [600], 50)
    check_rrr(oracle, X, out, 5, 1.0, 0.5, 600, 50, replicas={0, 4})


# ---- cut and resumed runs, two shards ---------------------------------------------------------------------------------------------------
def _cut_points(oracle, X, beta, thr, iters):
    """iterations after which the restatement's chain 0 has trefresh = max(N, 100) - 1, has just refreshed, and has just rejected a direct move"""
    with_tref, after_refresh, after_reject = [], [], []
    state = {"acc": 0, "ref": 0}

    def after(run):
        if run.ds.trefresh == max(X.N, 100) - 1:
            with_tref.append(run.it)
        if run.ds.refreshes > state["ref"]:
            after_refresh.append(run.it)
        if run.accepted == state["acc"] and run.acc_rate >= thr:
            after_reject.append(run.it)
        state["acc"], state["ref"] = run.accepted, run.ds.refreshes
    return with_tref, after_refresh, after_reject, after


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("name,sub", [("sat33", 1), ("perc", 0), ("skn", 1)])
def test_cut_and_resumed_runs_equal_the_run_in_one_call(pkg, oracle, name, sub, build):
    beta, thr, iters, step, R = 1.0, 0.5, 600, 7, 3
    X = wrap(pkg, sub, name)
    whole = run_rrr(pkg, X, R, beta, thr, build, [iters], step)
    s = RE.config_from_chunks(whole["C0"].s[0], X.N)
    run = AF.AfRun(AF.reference_of(X), s, beta, SEED, oracle, replica=0, staged_thr=thr)
    a, b, c, after = _cut_points(oracle, X, beta, thr, iters)
    run.run(iters, step, after=after)
    assert a and b and c                                                          # every kind of cut point occurs in this run
    cuts = sorted({1, a[0], b[0], c[0], c[len(c) // 2]} - {iters})
    pieces = [y - x for x, y in zip([0] + cuts, cuts + [iters])]
    cut = run_rrr(pkg, X, R, beta, thr, build, pieces, step)
    two = run_rrr(pkg, X, R + 64, beta, thr, build, [iters], step, devices=[0, 0])
    one = run_rrr(pkg, X, R + 64, beta, thr, build, [iters], step)
    for k in ("Es", "acc", "staged", "Etr"):
        assert (whole[k] == cut[k]).all(), k
        assert (one[k] == two[k]).all(), k
        assert (one[k][:R] == whole[k]).all(), k
    assert (whole["C1"].s == cut["C1"].s).all() and (one["C1"].s == two["C1"].s).all()
    for x, y, z in zip(whole["cache"], cut["cache"], one["cache"]):
        assert (x == y).all() and (z[:R] == x).all()
    for x, y in zip(one["cache"], two["cache"]):
        assert (x == y).all()


# ---- standardMC -------------------------------------------------------------------------------------------------------------------------
def _standard(pkg, X, R, beta, iters, step, pieces=None):
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(SEED)
        eng.init_spins_random()
        C0 = eng.get_config()
        Es, acc = [], np.zeros(R, np.int64)
        for k, n in enumerate(pieces or [iters]):
            eng.set_resume(k > 0)
            e, a = eng.standard_mc(beta, n, step)
            Es.append(np.atleast_2d(e))
            acc += a
        eng.set_resume(False)
        return C0, np.concatenate(Es, axis=1), acc, eng.get_config(), np.atleast_1d(eng.run_energy())


@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
@pytest.mark.parametrize("name", ["sat33", "perc", "skn", "commqu", "empty9"])
def test_standard_mc_bit_exact(pkg, oracle, name, sub):
    beta, iters, step, R = 0.8, 1000, 50, 33
    X = wrap(pkg, sub, name)
    C0, Es, acc, C1, Etr = _standard(pkg, X, R, beta, iters, step)
    cut = _standard(pkg, X, R, beta, iters, step, pieces=[50, 450, 500])
    assert (cut[1] == Es).all() and (cut[2] == acc).all() and (cut[3].s == C1.s).all() and (cut[4] == Etr).all()
    for r in (0, R - 1):
        s = RE.config_from_chunks(C0.s[r], X.N)
        es, E, a = AF.standard_mc(AF.reference_of(X), s, beta, iters, step, SEED, oracle, replica=r)
        assert Es[r].tolist() == es and acc[r] == a and Etr[r] == E, r
        assert (C1.s[r] == RE.chunks_from_config(s)).all(), r


@pytest.mark.parametrize("name,make", [("sat33", lambda pkg, g: pkg.GraphAddSubFields(fields(g.N), g)),
                                       ("perc", lambda pkg, g: pkg.GraphAddFields(np.zeros(g.N), g))], ids=["AddSubFields-SAT", "AddFields-zeros-PercStep"])
def test_standard_mc_equals_the_stand_alone_engine(pkg, name, make):
    g = graph(pkg, name)
    a = _standard(pkg, make(pkg, g), 40, 1.3, 2000, 100)
    b = _standard(pkg, g, 40, 1.3, 2000, 100)
    assert (a[0].s == b[0].s).all() and (a[3].s == b[3].s).all() and (a[2] == b[2]).all()
    assert (a[1] == b[1]).all() and (a[4] == b[4]).all()                           # Es and the tracked E equal as floats


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_what_is_not_wired_is_refused(pkg):
    X = wrap(pkg, 1, "sat33")
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call, word in ((lambda: eng.bkl_mc(1.0, 10), "bklMC"), (lambda: eng.wtm_mc(1.0, 2), "wtmMC"), (lambda: eng.extremal_opt(1.2, 10), "extremal_opt")):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3 and word in str(e.value) and "GraphAddSubFields" in str(e.value)
        h = fields(33)
        h[3] = np.nan
        rc = pkg.lib().rrrmc_af_set_fields(eng._ctx, h)
        assert rc == 1 and b"finite" in pkg.lib().rrrmc_last_error(eng._ctx)
        eng.rrr_mc(1.0, 10)                                                       # the fields it had still stand
    with pytest.raises(TypeError, match="sparse graphs"):
        pkg.GraphAddFields(np.zeros(16), pkg.GraphRRG(16, 3))
    with pytest.raises(TypeError, match="ensembles"):
        pkg.GraphAddSubFields(np.zeros(9), pkg.Graph0RE(3, 3, 0.5, 1.0))
    with pytest.raises(ValueError, match="incompatible length"):
        pkg.GraphAddFields(np.zeros(5), graph(pkg, "perc"))


def test_the_stand_alone_graphs_keep_refusing_rrr_mc(pkg):
    with pkg.Engine(graph(pkg, "sat33"), 1) as eng:
        eng.seed(1)
        eng.init_spins_random()
        with pytest.raises(pkg.RRRMCError) as e:
            eng.rrr_mc(1.0, 10)
        assert e.value.code == 3
