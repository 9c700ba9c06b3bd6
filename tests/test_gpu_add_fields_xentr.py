"""GPU parity for GraphAddFields / GraphAddSubFields over GraphPercXEntr(33, 70, λ) — the wrappers are what opens rrrMC on the
cross-entropy perceptron —: rrrMC and standardMC equal tests/add_fields_reference.py driving the restatement (tests/xentr_reference.py)
bit for bit — sampled energies, the configuration, accepted and staged counts, the tracked energy and the DeltaECacheCont of
``Engine.af_cache()`` — through the LDS build and the forced global-memory build, with the debug checks on; a resumed run equals the run
made in one call."""
import os

import numpy as np
import pytest

import add_fields_reference as AF
import re_reference as RE
import xentr_reference as XR
from test_gpu_perc_xentr import bits

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 1, 2
SEED, N, P, R = 70417, 33, 70, 3
BETA, ITERS, STEP = 1.0, 600, 50          # max(N, 100)-spaced refreshes of the sampler's tree fall inside the run


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


def fields():
    h = np.random.default_rng(5).normal(size=N)
    h[0], h[N // 2] = 0.0, -0.0
    return h


def wrap(pkg, sub, lam):
    g = pkg.GraphPercXEntr(N, P, lam, seed=3)
    return (pkg.GraphAddSubFields if sub else pkg.GraphAddFields)(fields(), g)


def reference_of(X):
    return AF.AddFields(X.fields, XR.PercXEntrRef(X.X1.patterns(), Hs=X.X1.Hs), type(X).__name__ == "GraphAddSubFields")


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.5], ids=["direct", "default", "staged"])
@pytest.mark.parametrize("lam", [0.8, 6.0])
@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
def test_rrr_mc_bit_exact(pkg, oracle, sub, lam, thr, build):
    X = wrap(pkg, sub, lam)
    with _env(build), pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(SEED)
        eng.init_spins_random()
        C0 = eng.get_config().s.copy()
        E0 = eng.energy()
        Es, acc, st = eng.rrr_mc(BETA, ITERS, STEP, staged_thr=thr)
        assert eng.af_build() == build
        C1, Etr, cache, se = eng.get_config().s.copy(), eng.run_energy(), eng.af_cache(), eng.step_energy()
    for r in range(R):
        s = RE.config_from_chunks(C0[r], N)
        run = AF.AfRun(reference_of(X), s, BETA, SEED, oracle, replica=r, staged_thr=thr)
        assert bits(E0[r]) == bits(run.E), r
        es = run.run(ITERS, STEP)
        assert (bits(Es[r]) == bits(es)).all(), r
        assert acc[r] == run.accepted and st[r] == run.staged_its and run.accepted > 10, r
        assert (C1[r] == RE.chunks_from_config(s)).all(), r
        assert bits(Etr[r]) == bits(run.E), r
        dEs, v, z, tref = run.cache_view()
        assert (bits(cache[0][r]) == bits(dEs)).all() and (bits(cache[1][r]) == bits(v)).all(), r
        assert bits(cache[2][r]) == bits(z) and cache[3][r] == tref, r
        fresh = XR.PercXEntrRef(X.X1.patterns(), Hs=X.X1.Hs)
        fresh.energy(s)
        assert se[r] == fresh.step_energy()
        assert lam > 1 or run.ds.refreshes >= 1          # (at λ = 6 few moves are accepted: setindex! may not reach its refresh)


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
def test_standard_mc_bit_exact(pkg, oracle, sub, build):
    X = wrap(pkg, sub, 0.8)
    with _env(build), pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(SEED)
        eng.init_spins_random()
        C0 = eng.get_config().s.copy()
        Es, acc = eng.standard_mc(BETA, 1500, STEP)
        C1, Etr = eng.get_config().s.copy(), eng.run_energy()
    for r in range(R):
        s = RE.config_from_chunks(C0[r], N)
        es, E, a = AF.standard_mc(reference_of(X), s, BETA, 1500, STEP, SEED, oracle, replica=r)
        assert (bits(Es[r]) == bits(es)).all() and acc[r] == a and a > 10
        assert (C1[r] == RE.chunks_from_config(s)).all() and bits(Etr[r]) == bits(E)
    if sub:          # GraphAddSubFields under standardMC is the chain of g: the stand-alone engine's, in whichever build it takes
        with pkg.Engine(X.X1, R) as eng:
            eng.seed(SEED)
            eng.init_spins_random()
            Es2, acc2 = eng.standard_mc(BETA, 1500, STEP)
            assert (bits(Es2) == bits(Es)).all() and (acc2 == acc).all() and (eng.get_config().s == C1).all()


@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, sampler):
    X = wrap(pkg, 0, 0.8)
    pieces = [137, 1, 262, 200]
    with pkg.Engine(X, R) as a, pkg.Engine(X, R) as b:
        for e in (a, b):
            e.set_debug_checks(True)
            e.seed(SEED)
            e.init_spins_random()
        call = (lambda e, n: e.rrr_mc(BETA, n, STEP)) if sampler == "rrr" else (lambda e, n: e.standard_mc(BETA, n, STEP) + (np.zeros(R, np.int64),))
        Ea, acca, sta = call(a, ITERS)
        b.set_resume(True)
        Es, acc, st = [], np.zeros(R, np.int64), np.zeros(R, np.int64)
        for n in pieces:
            e_, ac, s_ = call(b, n)
            Es.append(e_)
            acc += ac
            st += s_
        assert (acca == acc).all() and (sta == st).all()
        if sampler == "rrr":          # (the samples of a cut standardMC run fall at multiples of `step` of each piece)
            assert (bits(Ea) == bits(np.concatenate(Es, axis=1))).all()
            for x, y in zip(a.af_cache(), b.af_cache()):
                assert (bits(x) == bits(y)).all() if x.dtype == np.float64 else (x == y).all()
        assert (a.get_config().s == b.get_config().s).all() and (bits(a.run_energy()) == bits(b.run_energy())).all()


def test_a_new_table_and_unwired_samplers(pkg, oracle):
    X = wrap(pkg, 1, 0.5)
    Y = pkg.GraphPercXEntr(X.X1, 2.0)
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(SEED)
        eng.init_spins_random()
        eng.set_resume(True)
        eng.rrr_mc(BETA, 200, STEP)
        C0 = eng.get_config().s.copy()
        eng.set_loss_table(Y.Hs)                                   # ends the resumable run: a fresh start with the new table
        Es, acc, st = eng.rrr_mc(BETA, 300, STEP)
        for r in range(R):
            s = RE.config_from_chunks(C0[r], N)
            ref = AF.AddFields(X.fields, XR.PercXEntrRef(Y.patterns(), Hs=Y.Hs), True)
            run = AF.AfRun(ref, s, BETA, SEED, oracle, replica=r, it0=200)
            assert (bits(Es[r]) == bits(run.run(300, STEP))).all() and acc[r] == run.accepted
        for call in (lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0), lambda: eng.extremal_opt(1.4, 100, 10)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3
