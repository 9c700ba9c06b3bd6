"""GPU parity for random K-SAT (src/graphs/SAT.jl): standardMC on the stand-alone GraphSAT equals the plain-Python restatement with its
literal ClauseCache (tests/sat_reference.py) bit for bit, through the wavefront-per-replica build and the thread-per-replica build, with
``rrrmc_sat_build`` showing which ran; the two builds agree on every replica; cut, resumed and two-shard runs agree; the debug checks pass;
and what is not wired answers RRRMC_ERR_UNSUPPORTED."""
import ctypes as C
import os

import numpy as np
import pytest

import re_reference as RE
import sat_reference as SR

pytestmark = pytest.mark.gpu

THREAD, WAVE = 1, 2


def _with_env(env, fn):
    old = os.environ.get("RRRMC_SAT_NO_WAVE")
    os.environ.pop("RRRMC_SAT_NO_WAVE", None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        os.environ.pop("RRRMC_SAT_NO_WAVE", None)
        if old is not None:
            os.environ["RRRMC_SAT_NO_WAVE"] = old


def _graph(pkg, shape):
    if shape == "ragged":
        return pkg.GraphSAT.from_clauses(*SR.ragged_instance())
    return pkg.GraphSAT(*shape, seed=1000 + shape[0])


SHAPES = [(10, 3, 4.2), (31, 3, 4.2), (33, 5, 8.0), "ragged"]


def test_shapes_cover_what_they_claim(pkg):
    X = _graph(pkg, (33, 5, 8.0))
    assert X.M == 264 and np.mean([len(t) for t in X.T]) > 32          # more than 32 occurrences per variable on average
    X = _graph(pkg, "ragged")
    assert X.max_conn > 64 and min(len(t) for t in X.T) == 0           # two ballot passes; a variable with ΔE = 0 always


# the build rule (host_sat.hpp: kSatWaveMaxR; the measurement behind it is in profiles/r12/sat.md): wave up to WAVE_MAX_R replicas, thread beyond
WAVE_MAX_R = 16384


@pytest.mark.parametrize("R,env,build", [(1, {}, WAVE), (33, {}, WAVE), (33, {"RRRMC_SAT_NO_WAVE": "1"}, THREAD), (2049, {}, WAVE),
                                         (2049, {"RRRMC_SAT_NO_WAVE": "1"}, THREAD)])
@pytest.mark.parametrize("beta", [0.0, 2.0, 40.0])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_standard_mc_bit_exact(pkg, oracle, shape, beta, R, env, build):
    _bit_exact(pkg, oracle, shape, beta, R, env, build)


@pytest.mark.parametrize("R,build", [(WAVE_MAX_R, WAVE), (WAVE_MAX_R + 1, THREAD)])
def test_both_sides_of_the_build_rule_bit_exact(pkg, oracle, R, build):
    _bit_exact(pkg, oracle, (31, 3, 4.2), 2.0, R, {}, build)          # one shape pins the threshold: the default build on each side of it


def _bit_exact(pkg, oracle, shape, beta, R, env, build):
    seed, iters, step = 77123, 3000, 100
    X = _graph(pkg, shape)
    N = X.N

    def run():
        with pkg.Engine(X, R) as eng:
            eng.set_debug_checks(True)
            eng.seed(seed)
            eng.init_spins_random()
            assert eng.sat_build() == 0
            C0 = eng.get_config()
            E0 = np.atleast_1d(eng.energy())
            assert E0.dtype == np.int64
            Es, acc = eng.standard_mc(beta, iters, step)
            assert eng.sat_build() == build
            return C0, E0, np.atleast_2d(Es), np.atleast_1d(acc), eng.get_config(), np.atleast_1d(eng.run_energy())

    C0, E0, Es, acc, C1, Etr = _with_env(env, run)
    assert Es.shape == (R, iters // step) and Es.dtype == np.float64
    for r in sorted({0, 31, 32, R - 1} & set(range(R))):
        s = RE.config_from_chunks(C0.s[r], N)
        Xr = SR.ClauseCache(N, X.A, X.J)
        assert E0[r] == Xr.energy(s)
        es, E, a = SR.standard_mc(Xr, s, beta, iters, step, seed, oracle, replica=r)
        assert Es[r].tolist() == es and acc[r] == a, r
        assert (C1.s[r] == RE.chunks_from_config(s)).all(), r
        assert Etr[r] == E == SR.pure_energy(X.A, X.J, s), r


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_two_builds_agree_on_every_replica(pkg, shape):
    X = _graph(pkg, shape)

    def run(build):
        def go():
            with pkg.Engine(X, 64) as eng:
                eng.set_debug_checks(True)
                eng.seed(5)
                eng.init_spins_random()
                out = eng.standard_mc(1.5, 3000, 100) + eng.standard_mc(0.3, 1000, 7)
                assert eng.sat_build() == build
                return out + (eng.get_config().s.copy(), eng.run_energy())
        return go

    a, b = _with_env({}, run(WAVE)), _with_env({"RRRMC_SAT_NO_WAVE": "1"}, run(THREAD))
    for x, y in zip(a, b):
        assert (np.asarray(x) == np.asarray(y)).all()


@pytest.mark.parametrize("env", [{}, {"RRRMC_SAT_NO_WAVE": "1"}], ids=["wave", "thread"])
def test_two_calls_equal_one_and_two_shards_equal_one(pkg, env):
    X = _graph(pkg, (31, 3, 4.2))

    def run():
        with pkg.Engine(X, 70) as a, pkg.Engine(X, 70) as b, pkg.Engine(X, 70, devices=[0, 0]) as c:
            for e in (a, b, c):
                e.set_debug_checks(True)
                e.seed(31)
                e.init_spins_random()
            Ea, acca = a.standard_mc(2.0, 3000, 100)
            Ec, accc = c.standard_mc(2.0, 3000, 100)
            b.set_resume(True)
            E1, acc1 = b.standard_mc(2.0, 1000, 100)
            E2, acc2 = b.standard_mc(2.0, 2000, 100)
            assert (Ea == np.concatenate([E1, E2], axis=1)).all() and (acca == acc1 + acc2).all()      # 1000 + 2000 in two calls = 3000 in one
            assert (Ea == Ec).all() and (acca == accc).all()
            assert (a.get_config().s == b.get_config().s).all() and (a.get_config().s == c.get_config().s).all()
            assert (a.run_energy() == b.run_energy()).all() and (a.run_energy() == c.run_energy()).all()
            assert (a.run_energy() == a.energy()).all()
    _with_env(env, run)


def test_hooked_run_equals_unhooked(pkg):
    X = _graph(pkg, (10, 3, 4.2))
    Es0, C0 = pkg.standardMC(X, 2.0, 2000, step=100, seed=5, quiet=True, replicas=3)
    Es1, C1 = pkg.standardMC(X, 2.0, 2000, step=100, seed=5, quiet=True, replicas=3, hook=lambda *a: True)
    assert (np.asarray(Es0) == np.asarray(Es1)).all() and (C0.s == C1.s).all()


def test_unsupported_samplers_and_abi_refusals_on_a_live_context(pkg):
    L = pkg.lib()
    X = _graph(pkg, (10, 3, 4.2))
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call in (lambda: eng.rrr_mc(1.0, 100, 10), lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0),
                     lambda: eng.extremal_opt(1.4, 100, 10)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3 and "GraphSAT" in str(e.value)
        ctx = eng._ctx
        one = np.zeros(3, np.int8)
        assert L.rrrmc_set_clauses(ctx, 1, 3, np.array([-1, -1, -1], np.int32), one) == 1           # an empty clause
        assert L.rrrmc_set_clauses(ctx, 1, 3, np.array([0, 10, -1], np.int32), one) == 1            # a variable out of range
        assert L.rrrmc_set_clauses(ctx, 1, 3, np.array([1, 1, 2], np.int32), one) == 1              # a variable twice
        assert L.rrrmc_set_clauses(ctx, 1, 3, np.array([2, 1, 3], np.int32), one) == 1              # unsorted
        assert L.rrrmc_set_clauses(ctx, 1, 9, np.arange(9, dtype=np.int32), np.zeros(9, np.int8)) == 3      # nine literals
        assert L.rrrmc_set_couplings_bits(ctx, np.zeros(10, np.uint64)) == 2                        # not an SK context
        assert L.rrrmc_set_patterns(ctx, np.zeros(1, np.uint64), 1) == 2
        # a refused call leaves the clauses in place; a good one replaces them
        Es, _ = eng.standard_mc(2.0, 100, 100)
        assert L.rrrmc_set_clauses(ctx, 1, 3, np.array([0, 1, 2], np.int32), np.array([1, 1, 1], np.int8)) == 0
        eng.set_config(pkg.Config(10, 2, np.zeros((2, 1), np.uint64)))
        assert eng.energy().tolist() == [1, 1]
    with pkg.Engine(pkg.Graph0RE(11, 3, 1.0, 1.0), 2) as eng:
        assert L.rrrmc_set_clauses(eng._ctx, 1, 1, np.zeros(1, np.int32), np.zeros(1, np.int8)) == 2        # not a SAT context
        b = C.c_int32(0)
        assert L.rrrmc_sat_build(eng._ctx, C.byref(b)) == 2
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create(C.byref(ctx), 33, 10, 3, 2, 0, 0) == 3                                # rrrmc_ctx_create keeps refusing the model
    for X in (pkg.GraphSATRE(10, 3, 4.2, 3, 1.5, 2.0), pkg.GraphSATLE(10, 3, 4.2, 3, 1.5, 2.0)):
        with pkg.Engine(X, 2) as eng:
            eng.seed(1)
            eng.init_spins_random()
            for call in (lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0), lambda: eng.extremal_opt(1.4, 100, 10)):
                with pytest.raises(pkg.RRRMCError) as e:
                    call()
                assert e.value.code == 3
