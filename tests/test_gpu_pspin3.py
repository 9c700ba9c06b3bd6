"""GPU parity for the regular 3-spin model (src/graphs/PSpin3.jl): standardMC on the stand-alone GraphPSpin3 equals the plain-Python
restatement with its literal LocalFields{Int} cache (tests/pspin3_reference.py) bit for bit — sampled energies, accepted counts, final
chunks, tracked energy — through the wavefront-per-chain build (64 consecutive iterations side by side, retired in the chain's order) and
the thread-per-chain build, with ``rrrmc_pspin_build`` showing which ran; the two builds agree on every replica; cut, resumed and
two-shard runs agree; hooked runs equal unhooked ones; the debug checks stay on; the limits run and what lies beyond them, a broken table
and the four cache samplers are refused."""
import ctypes as C
import os

import numpy as np
import pytest

import pspin3_reference as PR
import re_reference as RE

pytestmark = pytest.mark.gpu

THREAD, WAVE = 1, 2
KEYS = ("RRRMC_PSPIN_NO_WAVE", "RRRMC_PSPIN_WAVE")


def _with_env(env, fn):
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


ENV = {THREAD: {"RRRMC_PSPIN_NO_WAVE": "1"}, WAVE: {"RRRMC_PSPIN_WAVE": "1"}}


def _doubled():
    l0 = [(0, 1, 2), (3, 4, 5), (6, 7, 8)]
    return 9, [l0, l0, [(0, 3, 6), (1, 4, 7), (2, 5, 8)]]          # one layer given twice: every pair of it counts twice


def _graph(pkg, shape):
    if shape == "doubled9":
        return pkg.GraphPSpin3.from_triples(*_doubled())
    return pkg.GraphPSpin3(*shape, seed=1000 + shape[0])


# (3, 1) one triple; (3, 2) every pair doubled, ΔE ∈ {±4}; (6, 3) nearly every batch lane conflicts with every accept; (33, 4) crosses a 32-bit
# word and has ΔE = 0 moves; (192, 16) the K limit, sparse conflicts
SHAPES = [(3, 1), (3, 2), (6, 3), (33, 4), (96, 5), (192, 16), "doubled9"]


def test_shapes_cover_what_they_claim(pkg):
    X = _graph(pkg, (3, 2))
    assert sorted(X.A[0].tolist()) == [1, 1, 2, 2]
    assert {abs(PR.pure_delta(X.A, s, i)) for s in ([0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]) for i in range(3)} == {4}
    X = _graph(pkg, (6, 3))
    assert all(len(set(a.tolist()) | {i}) == 5 for i, a in enumerate(X.A))          # a neighbourhood is 5 of the 6 sites: a later lane is hit by 5 accepts in 6
    X = _graph(pkg, (33, 4))
    s = np.random.default_rng(0).integers(0, 2, 33)
    assert {PR.pure_delta(X.A, s, i) for i in range(33)} == {-8, -4, 0, 4, 8}      # moves with ΔE = 0; spins beyond bit 31
    X = _graph(pkg, "doubled9")
    assert X.K == 3 and (X.A[:, 0:2] == X.A[:, 2:4]).all()


# the build rule (host_pspin.hpp: kPspinWaveMaxR): wave up to WAVE_MAX_R chains, thread beyond
WAVE_MAX_R = 16384


def _bit_exact(pkg, oracle, shape, beta, R, env, build, iters=3000, step=100):
    seed = 77123
    X = _graph(pkg, shape)
    N = X.N

    def run():
        with pkg.Engine(X, R) as eng:
            eng.set_debug_checks(True)
            eng.seed(seed)
            eng.init_spins_random()
            assert eng.pspin_build() == 0
            C0 = eng.get_config()
            E0 = np.atleast_1d(eng.energy())
            assert E0.dtype == np.int64
            Es, acc = eng.standard_mc(beta, iters, step)
            assert eng.pspin_build() == build
            return C0, E0, np.atleast_2d(Es), np.atleast_1d(acc), eng.get_config(), np.atleast_1d(eng.run_energy())

    C0, E0, Es, acc, C1, Etr = _with_env(env, run)
    assert Es.shape == (R, iters // step) and Es.dtype == np.float64
    for r in sorted({0, 31, 32, R - 1} & set(range(R))):
        s = RE.config_from_chunks(C0.s[r], N)
        Xr = PR.PSpin3Ref(N, X.A)
        assert E0[r] == Xr.energy(s)
        es, E, a = PR.standard_mc(Xr, s, beta, iters, step, seed, oracle, replica=r)
        assert Es[r].tolist() == es and acc[r] == a, r
        assert (C1.s[r] == RE.chunks_from_config(s)).all(), r
        assert Etr[r] == E == PR.pure_energy(X.A, s), r


@pytest.mark.parametrize("R,build", [(1, WAVE), (1, THREAD), (33, WAVE), (33, THREAD), (2049, WAVE), (2049, THREAD)])
@pytest.mark.parametrize("beta", [0.0, 2.0, 40.0])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_standard_mc_bit_exact(pkg, oracle, shape, beta, R, build):
    _bit_exact(pkg, oracle, shape, beta, R, ENV[build], build)


@pytest.mark.parametrize("build", [WAVE, THREAD])
@pytest.mark.parametrize("beta", [float("inf"), -1.0])
def test_infinite_and_negative_beta(pkg, oracle, beta, build):
    # β = +∞ with ΔE = 0 has x = NaN and is rejected, as the reference does; β < 0 is taken
    _bit_exact(pkg, oracle, (33, 4), beta, 33, ENV[build], build)


@pytest.mark.parametrize("build", [WAVE, THREAD])
@pytest.mark.parametrize("iters,step", [(10, 7), (10, 100), (3000, 7)])
@pytest.mark.parametrize("shape", [(6, 3), (33, 4)], ids=str)
def test_short_calls_tail_batches_and_step_7(pkg, oracle, shape, iters, step, build):
    # neither 10 nor 3000 is a multiple of 64: iters < 64, and a last batch of 56; step 7 samples several times inside one batch
    _bit_exact(pkg, oracle, shape, 2.0, 33, ENV[build], build, iters=iters, step=step)


@pytest.mark.parametrize("R,build", [(WAVE_MAX_R, WAVE), (WAVE_MAX_R + 1, THREAD)])
def test_both_sides_of_the_build_rule_bit_exact(pkg, oracle, R, build):
    _bit_exact(pkg, oracle, (33, 4), 2.0, R, {}, build)             # one shape pins the threshold: the default build on each side of it


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
                assert eng.pspin_build() == build
                return out + (eng.get_config().s.copy(), eng.run_energy())
        return go

    a, b = _with_env(ENV[WAVE], run(WAVE)), _with_env(ENV[THREAD], run(THREAD))
    for x, y in zip(a, b):
        assert (np.asarray(x) == np.asarray(y)).all()


@pytest.mark.parametrize("build", [WAVE, THREAD], ids=["wave", "thread"])
def test_two_calls_equal_one_and_two_shards_equal_one(pkg, build):
    X = _graph(pkg, (33, 4))

    def run():
        with pkg.Engine(X, 70) as a, pkg.Engine(X, 70) as b, pkg.Engine(X, 70, devices=[0, 0]) as c:
            for e in (a, b, c):
                e.set_debug_checks(True)
                e.seed(31)
                e.init_spins_random()
            Ea, acca = a.standard_mc(2.0, 3000, 100)
            Ec, accc = c.standard_mc(2.0, 3000, 100)
            assert c.pspin_build() == build
            b.set_resume(True)
            E1, acc1 = b.standard_mc(2.0, 1000, 100)
            E2, acc2 = b.standard_mc(2.0, 2000, 100)
            assert (Ea == np.concatenate([E1, E2], axis=1)).all() and (acca == acc1 + acc2).all()      # 1000 + 2000 in two calls = 3000 in one
            assert (Ea == Ec).all() and (acca == accc).all()
            assert (a.get_config().s == b.get_config().s).all() and (a.get_config().s == c.get_config().s).all()
            assert (a.run_energy() == b.run_energy()).all() and (a.run_energy() == c.run_energy()).all()
            assert (a.run_energy() == a.energy()).all()
    _with_env(ENV[build], run)


def test_hooked_run_equals_unhooked_and_a_hook_stops_one_replica(pkg):
    X = _graph(pkg, (33, 4))
    Es0, C0 = pkg.standardMC(X, 2.0, 2000, step=100, seed=5, quiet=True, replicas=3)
    Es1, C1 = pkg.standardMC(X, 2.0, 2000, step=100, seed=5, quiet=True, replicas=3, hook=lambda *a: True)
    assert (np.asarray(Es0) == np.asarray(Es1)).all() and (C0.s == C1.s).all()
    at = {}

    def hook(it, X_, Cfg, acc, E):
        if it == 600:
            at["s"] = Cfg.s[1].copy()
        return np.array([True, it < 600, True])

    Es2, C2 = pkg.standardMC(X, 2.0, 2000, step=100, seed=5, quiet=True, replicas=3, hook=hook)
    assert len(Es2[0]) == 20 and len(Es2[1]) == 6 and len(Es2[2]) == 20
    assert list(Es2[1]) == list(np.asarray(Es0)[1][:6]) and list(Es2[0]) == list(np.asarray(Es0)[0]) and list(Es2[2]) == list(np.asarray(Es0)[2])
    assert (C2.s[1] == at["s"]).all() and (C2.s[0] == C0.s[0]).all() and (C2.s[2] == C0.s[2]).all()


@pytest.mark.parametrize("N,K,build", [(65535, 2, WAVE), (65535, 2, THREAD), (300, 16, WAVE), (300, 16, THREAD)])
def test_the_limits_run_once(pkg, oracle, N, K, build):
    seed, iters, step, R = 9, 200, 50, 2
    X = pkg.GraphPSpin3(N, K, seed=3)

    def run():
        with pkg.Engine(X, R) as eng:
            eng.set_debug_checks(True)
            eng.seed(seed)
            eng.init_spins_random()
            C0 = eng.get_config()
            Es, acc = eng.standard_mc(0.5, iters, step)
            assert eng.pspin_build() == build
            return C0, np.atleast_2d(Es), np.atleast_1d(acc), eng.get_config(), np.atleast_1d(eng.run_energy()), np.atleast_1d(eng.energy())

    C0, Es, acc, C1, Etr, E1 = _with_env(ENV[build], run)
    assert (Etr == E1).all()
    s = RE.config_from_chunks(C0.s[1], N)
    Xr = PR.PSpin3Ref(N, X.A)
    es, E, a = PR.standard_mc(Xr, s, 0.5, iters, step, seed, oracle, replica=1)
    assert Es[1].tolist() == es and acc[1] == a and Etr[1] == E
    assert (C1.s[1] == RE.chunks_from_config(s)).all()


def test_refusals_on_a_device(pkg):
    L = pkg.lib()
    INVALID, STATE, UNSUPPORTED = 1, 2, 3
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create_pspin3(C.byref(ctx), 6, 17, 0, 2, 0, 0) == UNSUPPORTED                # K = 17
    assert L.rrrmc_ctx_create_pspin3(C.byref(ctx), 7, 3, 0, 2, 0, 0) == UNSUPPORTED                 # N % 3 != 0
    assert L.rrrmc_ctx_create_pspin3(C.byref(ctx), 65538, 3, 0, 2, 0, 0) == UNSUPPORTED
    assert L.rrrmc_ctx_create(C.byref(ctx), 105, 6, 3, 2, 0, 0) != 0                                # rrrmc_ctx_create does not make the model
    X = _graph(pkg, (6, 3))
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call in (lambda: eng.rrr_mc(1.0, 100, 10), lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0),
                     lambda: eng.extremal_opt(1.4, 100, 10)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == UNSUPPORTED and "GraphPSpin3" in str(e.value) and "GraphAddFields / GraphAddSubFields" in str(e.value)
        ctx = eng._ctx
        A = X.A.copy()
        assert L.rrrmc_set_pspin3(ctx, None) == INVALID
        for e, v in ((0, 6), (0, -1), (0, int(A[0, 1])), (0, 0)):                                   # out of range twice, partners equal, a partner is i
            B = A.copy().reshape(-1)
            B[e] = v
            assert L.rrrmc_set_pspin3(ctx, B) == INVALID
        B = A.copy()
        B[0, 0] = next(j for j in range(1, 6) if j not in (A[0, 0], A[0, 1]))                       # well formed, but the partners do not return it
        assert L.rrrmc_set_pspin3(ctx, B.reshape(-1)) == INVALID and "not consistent" in L.rrrmc_last_error(ctx).decode()
        assert L.rrrmc_set_couplings_bits(ctx, np.zeros(6, np.uint64)) == STATE                     # not an SK context
        assert L.rrrmc_set_clauses(ctx, 1, 1, np.zeros(1, np.int32), np.zeros(1, np.int8)) == STATE
        assert L.rrrmc_af_set_fields(ctx, np.zeros(6)) == STATE                                     # the stand-alone graph has no fields
        # a refused upload leaves the table in place; a good one replaces it
        Es, _ = eng.standard_mc(2.0, 100, 100)
        Y = pkg.GraphPSpin3.from_triples(6, [[(0, 1, 2), (3, 4, 5)]] * 3)
        assert L.rrrmc_set_pspin3(ctx, Y.A.reshape(-1)) == 0
        eng.set_config(pkg.Config(6, 2, np.array([[0b111111], [0b000111]], np.uint64)))
        assert eng.energy().tolist() == [-6, 0]
    with pkg.Engine(pkg.Graph0RE(11, 3, 1.0, 1.0), 2) as eng:
        assert L.rrrmc_set_pspin3(eng._ctx, np.zeros(6, np.int32)) == STATE                         # not a 3-spin context
        b = C.c_int32(0)
        assert L.rrrmc_pspin_build(eng._ctx, C.byref(b)) == STATE
