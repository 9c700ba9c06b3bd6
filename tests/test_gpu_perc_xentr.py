"""GPU parity for the cross-entropy perceptron (src/graphs/PercXEntr.jl): standardMC on the stand-alone GraphPercXEntr equals the
plain-Python restatement (tests/xentr_reference.py) BIT FOR BIT — doubles are compared through their uint64 view — in both kernel builds
(one thread per chain, one wavefront per chain), each with the loss table in LDS and in global memory; resumed and hooked runs, a table
swapped between calls, two-shard contexts and the debug checks agree; step_energy matches; refusals are enforced."""
import ctypes as C
import os

import numpy as np
import pytest

import re_reference as RE
import xentr_reference as XR

pytestmark = pytest.mark.gpu

ENVS = ("RRRMC_XENTR_NO_WAVE", "RRRMC_XENTR_WAVE", "RRRMC_XENTR_NO_LDS")
BUILDS = [("thread", {"RRRMC_XENTR_NO_WAVE": "1"}, 1), ("thread-global-table", {"RRRMC_XENTR_NO_WAVE": "1", "RRRMC_XENTR_NO_LDS": "1"}, 1),
          ("wave", {"RRRMC_XENTR_WAVE": "1"}, 2), ("wave-global-table", {"RRRMC_XENTR_WAVE": "1", "RRRMC_XENTR_NO_LDS": "1"}, 2)]


def bits(x):
    """the uint64 view of Float64s: equality of these is equality bit for bit (−0.0 ≠ 0.0, NaN == NaN)"""
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


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


_REF = {}


def _reference(oracle, xi, Hs, N, seed, beta, iters, step, r, chunks):
    """the restatement's chain of replica r, computed once per case and shared by the four builds"""
    key = (N, xi.shape[0], Hs[0], seed, beta, iters, step, r)
    if key not in _REF:
        s = RE.config_from_chunks(chunks, N)
        X = XR.PercXEntrRef(xi, Hs=Hs)
        E0 = X.energy(s)
        es, E, a = XR.standard_mc(X, s, beta, iters, step, seed, oracle, replica=r, E=E0)
        _REF[key] = (E0, es, E, a, RE.chunks_from_config(s), X.step_energy())
    return _REF[key]


# (5, 3): a partial last pattern word; (33, 70): more than one pattern word; (129, 130): four spin words, a third pattern word of two patterns.
# R = 1: one chain; 3: a partial wavefront; 70: a second wavefront of the thread build.  λ = 6: many entries of the table are tiny
# (below 1e-6, and exactly 0.0 where 1 + exp(x) rounds to 1), all finite.
@pytest.mark.parametrize("lam", [0.8, 6.0])
@pytest.mark.parametrize("R", [1, 3, 70])
@pytest.mark.parametrize("N,P", [(5, 3), (33, 70), (129, 130)])
def test_standard_mc_bit_exact_in_all_four_builds(pkg, oracle, N, P, R, lam):
    seed, beta, iters, step = 9100 + N + R, 1.1, 2000, 100
    X = pkg.GraphPercXEntr(N, P, lam, seed=seed)
    xi, Hs = X.patterns(), X.Hs.tolist()
    assert np.isfinite(X.Hs).all() and (lam < 6 or (X.Hs < 1e-6).sum() >= 2)
    check = range(R) if R <= 3 else (0, 1, 63, 64, R - 1)
    outs = []
    for name, env, build in BUILDS:
        def run():
            with pkg.Engine(X, R) as eng:
                eng.set_debug_checks(True)
                eng.seed(seed)
                eng.init_spins_random()
                C0 = eng.get_config().s.copy()
                E0 = eng.energy()
                Es, acc = eng.standard_mc(beta, iters, step)
                assert eng.xentr_build() == build, name
                return C0, E0, Es, acc, eng.get_config().s.copy(), eng.run_energy(), eng.step_energy()
        outs.append(_with_env(env, run))
    C0, E0, Es, acc, C1, Etr, SE = outs[0]
    for o in outs[1:]:          # the four builds agree on every chain
        assert (o[0] == C0).all() and (bits(o[1]) == bits(E0)).all() and (bits(o[2]) == bits(Es)).all() and (o[3] == acc).all()
        assert (o[4] == C1).all() and (bits(o[5]) == bits(Etr)).all() and (o[6] == SE).all()
    for r in check:             # ... and with the restatement
        e0, es, E, a, ch, se = _reference(oracle, xi, Hs, N, seed, beta, iters, step, r, C0[r])
        assert bits(E0[r]) == bits(e0)
        assert (bits(Es[r]) == bits(es)).all() and acc[r] == a and a > 0
        assert (C1[r] == ch).all() and bits(Etr[r]) == bits(E) and SE[r] == se


def test_a_second_call_continues_the_streams_and_largest_shape_runs(pkg, oracle):
    # a fresh call after a call: the streams go on, E restarts from energy(X, C); then the shape the limits must admit, N = 1001, P = 400
    N, P, lam, seed, beta, R = 33, 70, 0.8, 77, 1.1, 3
    X = pkg.GraphPercXEntr(N, P, lam, seed=seed)
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config().s.copy()
        eng.standard_mc(beta, 500, 100)
        Es2, acc2 = eng.standard_mc(beta, 500, 100)
        for r in range(R):
            s = RE.config_from_chunks(C0[r], N)
            Xr = XR.PercXEntrRef(X.patterns(), Hs=X.Hs)
            XR.standard_mc(Xr, s, beta, 500, 100, seed, oracle, replica=r)
            es, E, a = XR.standard_mc(XR.PercXEntrRef(X.patterns(), Hs=X.Hs), s, beta, 500, 100, seed, oracle, replica=r, it0=500)
            assert (bits(Es2[r]) == bits(es)).all() and acc2[r] == a
    X = pkg.GraphPercXEntr(1001, 400, 1.0, seed=4)
    res = []
    for name, env, build in BUILDS:
        def run():
            with pkg.Engine(X, 2) as eng:
                eng.set_debug_checks(True)
                eng.seed(4)
                eng.init_spins_random()
                Es, acc = eng.standard_mc(2.0, 3000, 1000)
                Etr, E = eng.run_energy(), eng.energy()
                assert (np.abs(Etr - E) <= 1e-9).all() and (acc > 0).all()
                return bits(Es), acc, bits(Etr), eng.get_config().s.copy()
        res.append(_with_env(env, run))
    for o in res[1:]:
        assert all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(o, res[0]))


@pytest.mark.parametrize("build", [BUILDS[0], BUILDS[2]], ids=["thread", "wave"])
def test_resumed_hooked_and_sharded_runs(pkg, build):
    X = pkg.GraphPercXEntr(45, 80, 0.9, seed=9)

    def run():
        with pkg.Engine(X, 70) as a, pkg.Engine(X, 70) as b, pkg.Engine(X, 70, devices=[0, 0]) as c:
            for e in (a, b, c):
                e.set_debug_checks(True)
                e.seed(31)
                e.init_spins_random()
            Ea, acca = a.standard_mc(0.9, 2000, 50)
            Ec, accc = c.standard_mc(0.9, 2000, 50)            # a two-device context (both shards on device 0) is the single context
            assert a.xentr_build() == build[2] and c.xentr_build() == build[2]
            b.set_resume(True)
            acc = np.zeros(70, np.int64)
            for n in (350, 1, 649, 1000):                      # a run cut into resumed calls is the run in one call
                acc += b.standard_mc(0.9, n, 50)[1]
            assert (acca == acc).all() and (acca == accc).all() and (bits(Ea) == bits(Ec)).all()
            assert (a.get_config().s == b.get_config().s).all() and (a.get_config().s == c.get_config().s).all()
            assert (bits(a.run_energy()) == bits(b.run_energy())).all() and (bits(a.run_energy()) == bits(c.run_energy())).all()
            assert (a.step_energy() == c.step_energy()).all()
        Es0, C0 = pkg.standardMC(X, 0.9, 1000, step=100, seed=5, quiet=True, replicas=3)
        seen = []

        def hook(it, X_, Cfg, acc, E):
            se = pkg.step_energy(X_)                            # (of the live engine: replica 1 goes on there after the hook froze it)
            for r in (0, 2):
                ref = XR.PercXEntrRef(X.patterns(), Hs=X.Hs)
                assert abs(ref.energy(RE.config_from_chunks(Cfg.s[r], X.N)) - E[r]) < 1e-10
                assert se[r] == ref.step_energy()
            seen.append(it)
            return np.array([True, it < 500, True])             # the hook stops replica 1 at iteration 500

        Es1, C1 = pkg.standardMC(X, 0.9, 1000, step=100, seed=5, quiet=True, replicas=3, hook=hook)
        assert seen == list(range(100, 1001, 100))
        Es0 = np.asarray(Es0)
        assert (bits(Es1[0]) == bits(Es0[0])).all() and (bits(Es1[2]) == bits(Es0[2])).all() and (C0.s[[0, 2]] == C1.s[[0, 2]]).all()
        assert len(Es1[1]) == 5 and (bits(Es1[1]) == bits(Es0[1][:5])).all()
    _with_env(build[1], run)


@pytest.mark.parametrize("build", [BUILDS[0], BUILDS[2]], ids=["thread", "wave"])
def test_a_new_table_between_calls_restarts_from_its_energy(pkg, oracle, build):
    # GraphPercXEntr(X, λnew) on fixed patterns: rrrmc_set_loss_table ends the resumable run, the next call starts from energy(X, C) of the new table
    N, P, seed, beta, R = 33, 70, 515, 1.0, 3
    X = pkg.GraphPercXEntr(N, P, 0.5, seed=seed)
    Y = pkg.GraphPercXEntr(X, 2.0)

    def run():
        with pkg.Engine(X, R) as eng:
            eng.set_debug_checks(True)
            eng.seed(seed)
            eng.init_spins_random()
            C0 = eng.get_config().s.copy()
            eng.set_resume(True)
            Es1, acc1 = eng.standard_mc(beta, 600, 100)
            eng.set_loss_table(Y.Hs)
            Es2, acc2 = eng.standard_mc(beta, 600, 100)
            return C0, Es1, acc1, Es2, acc2, eng.get_config().s.copy(), eng.run_energy()
    C0, Es1, acc1, Es2, acc2, C1, Etr = _with_env(build[1], run)
    for r in range(R):
        s = RE.config_from_chunks(C0[r], N)
        es1, _, a1 = XR.standard_mc(XR.PercXEntrRef(X.patterns(), Hs=X.Hs), s, beta, 600, 100, seed, oracle, replica=r)
        es2, E, a2 = XR.standard_mc(XR.PercXEntrRef(X.patterns(), Hs=Y.Hs), s, beta, 600, 100, seed, oracle, replica=r, it0=600)
        assert (bits(Es1[r]) == bits(es1)).all() and acc1[r] == a1 and (bits(Es2[r]) == bits(es2)).all() and acc2[r] == a2
        assert (C1[r] == RE.chunks_from_config(s)).all() and bits(Etr[r]) == bits(E)


def test_refusals(pkg):
    L = pkg.lib()
    X = pkg.GraphPercXEntr(11, 5, 1.0)
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call in (lambda: eng.rrr_mc(1.0, 100, 10), lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0),
                     lambda: eng.extremal_opt(1.4, 100, 10)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3
        for bad in (np.inf, -np.inf, np.nan):                      # a non-finite table is refused, the old one stays
            Hs = X.Hs.copy()
            Hs[3] = bad
            assert L.rrrmc_set_loss_table(eng._ctx, Hs, len(Hs)) == 1
        assert L.rrrmc_set_loss_table(eng._ctx, X.Hs[:-1].copy(), len(X.Hs) - 1) == 1          # n must be N + 1
        eng.standard_mc(1.0, 100, 10)
        assert L.rrrmc_set_couplings_bits(eng._ctx, np.zeros(11, np.uint64)) == 2
    # a sampling call before the table is set is refused, as calls before rrrmc_set_patterns are
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create_perc_xentr(C.byref(ctx), 11, 2, 0, 0) == 0
    try:
        assert L.rrrmc_standard_mc_async(ctx, 1.0, 10, 1) == 2 and b"rrrmc_set_graph has not been called" in L.rrrmc_last_error(ctx)
        assert L.rrrmc_set_patterns(ctx, X.xi.reshape(-1), X.P) == 0
        assert L.rrrmc_standard_mc_async(ctx, 1.0, 10, 1) == 2 and b"rrrmc_set_loss_table" in L.rrrmc_last_error(ctx)
        assert L.rrrmc_energy_f64(ctx, np.zeros(2)) == 2
        assert L.rrrmc_set_loss_table(ctx, X.Hs, len(X.Hs)) == 0
        assert L.rrrmc_seed(ctx, 3) == 0 and L.rrrmc_init_spins_random(ctx) == 0
        assert L.rrrmc_standard_mc_async(ctx, 1.0, 10, 1) == 0 and L.rrrmc_sync(ctx) == 0
    finally:
        L.rrrmc_ctx_destroy(ctx)
    with pkg.Engine(pkg.GraphPercStep(11, 5), 2) as eng:
        assert L.rrrmc_set_loss_table(eng._ctx, X.Hs, len(X.Hs)) == 2      # not a GraphPercXEntr context
        b = C.c_int32(0)
        assert L.rrrmc_xentr_build(eng._ctx, C.byref(b)) == 2
