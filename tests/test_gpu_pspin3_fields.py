"""GPU parity for GraphAddFields / GraphAddSubFields over a GraphPSpin3: rrrMC and standardMC equal the plain-Python restatement
(tests/add_fields_reference.py with the literal LocalFields{Int} cache of tests/pspin3_reference.py as g) bit for bit — spins, sampled
energies, accepted and staged counts and the DeltaECacheCont that ``rrrmc_af_cache`` returns — through the LDS build and the forced
global-memory build, with ``rrrmc_af_build`` showing which ran; cut, resumed and two-shard runs equal the run made in one call; standardMC
on GraphAddSubFields equals the stand-alone engine.  The debug checks are on in every run."""
import os

import numpy as np
import pytest

import add_fields_reference as AF
import pspin3_reference as PR
import re_reference as RE

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 1, 2
SEED = 90417
SHAPES = [(6, 3), (33, 4), (96, 5)]


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


def wrap(pkg, sub, shape):
    g = pkg.GraphPSpin3(*shape, seed=1000 + shape[0])
    return (pkg.GraphAddSubFields if sub else pkg.GraphAddFields)(fields(g.N), g)


def reference_of(X):
    return AF.AddFields(X.fields, PR.PSpin3Ref(X.N, X.X1.A), type(X).__name__ == "GraphAddSubFields")


def run_rrr(pkg, X, R, beta, thr, build, pieces, step, devices=None):
    """an rrrMC run made of the given pieces (resumed calls) from random spins: what the engine hands back"""
    with _env(build), pkg.Engine(X, R, devices=devices) as eng:
        eng.set_debug_checks(True)
        eng.seed(SEED)
        eng.init_spins_random()
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
        run = AF.AfRun(reference_of(X), s, beta, SEED, oracle, replica=r, staged_thr=thr)
        assert out["E0"][r] == run.E, r
        es = run.run(iters, step)
        assert out["Es"][r].tolist() == es, r
        assert out["acc"][r] == run.accepted and out["staged"][r] == run.staged_its, r
        assert (out["C1"].s[r] == RE.chunks_from_config(s)).all(), r
        assert out["Etr"][r] == run.E, r
        dEs, v, z, tref = run.cache_view()
        assert out["cache"][0][r].tolist() == dEs and out["cache"][1][r].tolist() == v, r              # af_cache()
        assert out["cache"][2][r] == z and out["cache"][3][r] == tref, r
    return run


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.5], ids=["direct", "default", "staged"])
@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_rrr_mc_bit_exact(pkg, oracle, shape, sub, thr, beta, build):
    iters, step, R = 600, 50, 33 if shape == (33, 4) else 3
    X = wrap(pkg, sub, shape)
    out = run_rrr(pkg, X, R, beta, thr, build, [iters], step)
    assert out["Es"].shape == (R, iters // step) and out["Es"].dtype == np.float64
    run = check_rrr(oracle, X, out, R, beta, thr, iters, step)
    if thr == 0.0:
        assert run.staged_its == 0
    if thr == 1.5:
        assert run.staged_its == iters


@pytest.mark.parametrize("shape,sub", [((6, 3), 0), ((33, 4), 1), ((96, 5), 0)], ids=str)
def test_the_lds_build_and_the_global_build_agree(pkg, shape, sub):
    X = wrap(pkg, sub, shape)
    a = run_rrr(pkg, X, 40, 0.8, 0.5, LDS, [600, 150], 7)
    b = run_rrr(pkg, X, 40, 0.8, 0.5, GLOBAL, [600, 150], 7)
    for k in ("E0", "Es", "acc", "staged", "Etr"):
        assert (a[k] == b[k]).all(), k
    assert (a["C1"].s == b["C1"].s).all()
    for x, y in zip(a["cache"], b["cache"]):
        assert (x == y).all()


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
def test_cut_and_resumed_runs_and_two_shards_equal_the_run_in_one_call(pkg, oracle, build):
    beta, thr, iters, step, R = 1.0, 0.5, 600, 7, 3
    X = wrap(pkg, 1, (33, 4))
    whole = run_rrr(pkg, X, R, beta, thr, build, [iters], step)
    cut = run_rrr(pkg, X, R, beta, thr, build, [1, 99, 100, 37, 363], step)
    two = run_rrr(pkg, X, R + 64, beta, thr, build, [iters], step, devices=[0, 0])
    for k in ("Es", "acc", "staged", "Etr"):
        assert (whole[k] == cut[k]).all(), k
        assert (two[k][:R] == whole[k]).all(), k
    assert (whole["C1"].s == cut["C1"].s).all() and (two["C1"].s[:R] == whole["C1"].s).all()
    for x, y, z in zip(whole["cache"], cut["cache"], two["cache"]):
        assert (x == y).all() and (z[:R] == x).all()
    check_rrr(oracle, X, whole, R, beta, thr, iters, step, replicas={0, 2})


def _standard(pkg, X, R, beta, iters, step, pieces=None, devices=None):
    with pkg.Engine(X, R, devices=devices) as eng:
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
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_standard_mc_bit_exact(pkg, oracle, shape, sub):
    beta, iters, step, R = 0.8, 1000, 50, 33
    X = wrap(pkg, sub, shape)
    C0, Es, acc, C1, Etr = _standard(pkg, X, R, beta, iters, step)
    cut = _standard(pkg, X, R, beta, iters, step, pieces=[50, 450, 500])
    two = _standard(pkg, X, R + 64, beta, iters, step, devices=[0, 0])
    assert (cut[1] == Es).all() and (cut[2] == acc).all() and (cut[3].s == C1.s).all() and (cut[4] == Etr).all()
    assert (two[1][:R] == Es).all() and (two[2][:R] == acc).all() and (two[3].s[:R] == C1.s).all() and (two[4][:R] == Etr).all()
    for r in (0, R - 1):
        s = RE.config_from_chunks(C0.s[r], X.N)
        es, E, a = AF.standard_mc(reference_of(X), s, beta, iters, step, SEED, oracle, replica=r)
        assert Es[r].tolist() == es and acc[r] == a and Etr[r] == E, r
        assert (C1.s[r] == RE.chunks_from_config(s)).all(), r


def test_standard_mc_on_add_sub_fields_equals_the_stand_alone_engine(pkg):
    g = pkg.GraphPSpin3(33, 4, seed=1033)
    a = _standard(pkg, pkg.GraphAddSubFields(fields(33), g), 40, 1.3, 2000, 100)
    b = _standard(pkg, g, 40, 1.3, 2000, 100)
    assert (a[0].s == b[0].s).all() and (a[3].s == b[3].s).all() and (a[2] == b[2]).all()
    assert (a[1] == b[1]).all() and (a[4] == b[4]).all()                           # Es and the tracked E equal as floats


def test_what_is_not_wired_is_refused(pkg):
    X = wrap(pkg, 1, (6, 3))
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call, word in ((lambda: eng.bkl_mc(1.0, 10), "bklMC"), (lambda: eng.wtm_mc(1.0, 2), "wtmMC"), (lambda: eng.extremal_opt(1.2, 10), "extremal_opt")):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3 and word in str(e.value) and "GraphAddSubFields" in str(e.value)
        eng.rrr_mc(1.0, 10)
