"""CPU checks of random K-SAT (src/graphs/SAT.jl).  The first test validates the MODEL the engine is built on, inside tests/sat_reference.py
alone: ΔE written as a function of the configuration (what csrc/sat_core.hpp computes) equals the literal ClauseCache restated from the
reference after every step of a random walk — no library code runs in it (the library's own sat_delta is held to a direct clause count by
tests/sat_core_check.cpp, and to the literal cache by the GPU parity tests).  The others run library code: the host generator equals its
Python restatement; every refusal of the contract returns its code; the front end carries the reference's attributes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sat_reference as SR


def _instances(oracle):
    A, J = SR.gen_ksat(oracle, 10, 3, 4.2, 11)
    yield 10, A, J                                                     # 42 clauses (test/runtests.jl:68)
    A, J = SR.gen_ksat(oracle, 31, 3, 4.2, 12)
    yield 31, A, J                                                     # 130 clauses (test/runtests.jl:120)
    yield SR.ragged_instance()


def test_pure_delta_equals_the_literal_cache_over_a_random_walk(oracle):
    shapes = []
    for N, A, J in _instances(oracle):
        X = SR.ClauseCache(N, A, J)
        shapes.append((N, X.M, sorted({len(a) for a in A}), X.max_conn, min(len(t) for t in X.T)))
        rng = np.random.default_rng(N)
        s = rng.integers(0, 2, N)
        E = X.energy(s)
        assert E == SR.pure_energy(A, J, s)
        for _ in range(3000):
            i = int(rng.integers(N))
            d = SR.pure_delta(A, J, X.T, s, i)
            assert d == X.delta_energy(i)
            s[i] ^= 1
            X.update_cache(i)
            E += d
            assert E == SR.pure_energy(A, J, s)                        # E tracked by ΔE equals energy recounted
            assert all(X.delta_energy(j) == SR.pure_delta(A, J, X.T, s, j) for j in X.neighb[i])
        assert [X.delta_energy(j) for j in range(N)] == [SR.pure_delta(A, J, X.T, s, j) for j in range(N)]
        Y = SR.ClauseCache(N, A, J)                                    # the walked cache equals a fresh one, up to the order inside I
        assert Y.energy(s) == E and Y.S == X.S and Y.lfields == X.lfields
        assert [sorted(x[:n]) for x, n in zip(X.I, X.S)] == [sorted(y[:n]) for y, n in zip(Y.I, Y.S)]
    assert shapes[0][:2] == (10, 42) and shapes[1][:2] == (31, 130)
    N, M, lens, max_conn, min_conn = shapes[2]
    assert lens == list(range(1, 9)) and max_conn > 64 and min_conn == 0     # a unit clause, two ballot passes, a variable in no clause


@pytest.mark.parametrize("N,K,alpha,Mc", [(10, 3, 4.2, 42), (31, 3, 4.2, 130), (33, 5, 8.0, 264), (5, 1, 0.5, 2), (7, 2, 0.5, 4), (4, 4, 1.0, 4)])
def test_generator_equals_its_restatement(pkg, oracle, N, K, alpha, Mc):
    # α N exactly on a tie rounds to even, as Julia's round(Int, x) does: 2.5 -> 2, 3.5 -> 4
    for seed in (3, 167432777111):
        A, J = SR.gen_ksat(oracle, N, K, alpha, seed)
        assert len(A) == Mc
        m = C.c_int64(-1)
        assert pkg.lib().rrrmc_gen_ksat(N, K, alpha, seed, C.byref(m), None, None) == 0 and m.value == Mc
        X = pkg.GraphSAT(N, K, alpha, seed=seed)
        assert X.A == A and X.J == J and X.M == Mc and X.K == K and X.N == N
        for Aa in X.A:                                                 # sorted and distinct
            assert all(0 <= i < N for i in Aa) and all(x < y for x, y in zip(Aa, Aa[1:]))
    assert pkg.GraphSAT(31, 3, 4.2, seed=1).A != pkg.GraphSAT(31, 3, 4.2, seed=2).A


def _check(pkg, N, A, J, Kmax=None):
    Kmax = Kmax or max(max(len(a) for a in A), 1)
    v = np.full((len(A), Kmax), -1, np.int32)
    l = np.zeros((len(A), Kmax), np.int8)
    for a, (Aa, Ja) in enumerate(zip(A, J)):
        v[a, :len(Aa)] = Aa
        l[a, :len(Ja)] = Ja
    mc = C.c_int64(-1)
    return pkg.lib().rrrmc_check_clauses(N, len(A), Kmax, v.reshape(-1), l.reshape(-1), C.byref(mc)), mc.value


def test_every_refusal_of_the_contract_returns_its_code(pkg):
    L = pkg.lib()
    ctx = C.c_void_p()
    INVALID, UNSUPPORTED = 1, 3
    assert _check(pkg, 5, [[0, 2, 4], [1]], [[0, 1, 0], [1]]) == (0, 1)
    assert _check(pkg, 5, [[0, 1], []], [[0, 1], []])[0] == INVALID                    # an empty clause
    assert _check(pkg, 5, [[0, 5]], [[0, 1]])[0] == INVALID                            # a variable out of range
    assert _check(pkg, 5, [[1, 1, 2]], [[0, 1, 0]])[0] == INVALID                      # a variable twice in one clause
    assert _check(pkg, 5, [[2, 1]], [[0, 1]])[0] == INVALID                            # unsorted
    assert _check(pkg, 20, [list(range(8))], [[0] * 8]) == (0, 1)                      # len_a <= 8
    assert _check(pkg, 20, [list(range(9))], [[0] * 9])[0] == UNSUPPORTED
    assert _check(pkg, 65535, [[65534]], [[1]]) == (0, 1)                              # N <= 65 535
    assert _check(pkg, 65536, [[0]], [[1]])[0] == UNSUPPORTED
    assert L.rrrmc_ctx_create_sat(C.byref(ctx), 65536, 1, 0, 0) == UNSUPPORTED
    assert _check(pkg, 2, [[0]] * 65535, [[1]] * 65535) == (0, 65535)                  # |T[i]| <= 65 535
    assert _check(pkg, 2, [[0]] * 65536, [[1]] * 65536)[0] == UNSUPPORTED
    many = (1 << 20) + 1                                                               # Mc <= 2^20
    v = (np.arange(many, dtype=np.int32) % 60000).reshape(-1)
    assert L.rrrmc_check_clauses(60000, many - 1, 1, v[:-1].copy(), np.zeros(many - 1, np.int8), None) == 0
    assert L.rrrmc_check_clauses(60000, many, 1, v, np.zeros(many, np.int8), None) == UNSUPPORTED
    # under an ensemble, additionally the ensemble's own limits: M <= 32 (RE) / 31 (LE), 65 535 sites
    for create, big_m, sites in ((L.rrrmc_ctx_create_re, 33, (21846, 3)), (L.rrrmc_ctx_create_le, 32, (16384, 3))):
        assert create(C.byref(ctx), 10, big_m, 8, 1, 0, 0) == UNSUPPORTED
        assert create(C.byref(ctx), sites[0], sites[1], 8, 1, 0, 0) == UNSUPPORTED
        assert create(C.byref(ctx), 10, 2, 8, 1, 0, 0) == INVALID                      # M must be greater than 2
    # the generator's own checks (SAT.jl:43-46)
    m = C.c_int64(0)
    for N, K, alpha in ((0, 3, 1.0), (5, 0, 1.0), (5, 3, -0.5), (2, 3, 1.0)):
        assert L.rrrmc_gen_ksat(N, K, alpha, 1, C.byref(m), None, None) == INVALID
    # the front end refuses the same
    for A, J in (([[0, 1], []], [[0, 1], []]), ([[0, 5]], [[0, 1]]), ([[1, 1]], [[0, 1]]), ([[2, 1]], [[0, 1]]), ([[0]], [[0], [1]]), ([], [])):
        with pytest.raises(ValueError):
            pkg.GraphSAT.from_clauses(5, A, J)


def test_front_end_attributes(pkg, oracle, tmp_path):
    N, A, J = SR.ragged_instance()
    X = pkg.GraphSAT.from_clauses(N, A, J)
    R = SR.ClauseCache(N, A, J)
    assert (X.N, X.M, X.K, X.max_conn) == (R.N, R.M, R.K, R.max_conn) == (20, 90, 8, 70)
    assert X.A == R.A and X.J == R.J and X.T == R.T and X.neighb == R.neighb
    assert pkg.all_delta_e(X) == tuple(range(71))                                      # allΔE = 0 .. max_conn (SAT.jl:325)
    assert pkg.neighbors(X, 19).tolist() == [] and pkg.neighbors(X, 0).tolist() == R.neighb[0] and pkg.getN(X) == 20
    assert X.model_kind == 33 and X.energy_dtype == np.int64
    assert _check(pkg, N, A, J) == (0, 70)
    # the RE / LE constructors share one clause set, in both signatures
    Y = pkg.GraphSAT(10, 3, 4.2, seed=5)
    for ens, model in ((pkg.GraphSATRE, 34), (pkg.GraphSATLE, 35)):
        a, b = ens(Y, 3, 1.5, 2.0), ens(10, 3, 4.2, 3, 1.5, 2.0, seed=5)
        assert a.X1 is Y and b.X1.A == Y.A and b.X1.J == Y.J
        assert a.slice_kind == b.slice_kind == 8 and a.model_kind == b.model_kind == model
        assert a.Nk == 10 and a.M == 3 and a.N == (30 if model == 34 else 40)
        with pytest.raises(TypeError):
            ens(10, 3, 4.2, 3, 1.5)                                                    # neither signature
        with pytest.raises(TypeError):
            ens(pkg.GraphPercStep(11, 4), 3, 1.5, 2.0)
    # export_cnf (SAT.jl:129-140) round trip
    path = str(tmp_path / "x.cnf")
    X.export_cnf(path)
    lines = open(path).read().splitlines()
    assert lines[0] == "p cnf 20 90" and len(lines) == 91
    A2, J2 = [], []
    for ln in lines[1:]:
        toks = [int(t) for t in ln.split()]
        assert toks[-1] == 0 and ln.endswith(" 0")
        A2.append([abs(t) - 1 for t in toks[:-1]])
        J2.append([int(t > 0) for t in toks[:-1]])
    assert A2 == A and J2 == J


def test_small_instance_has_the_energy_levels_the_boltzmann_test_needs(pkg):
    # the instance of tests/test_gpu_sat_boltzmann.py: N = 9, 20 three-literal clauses
    X = pkg.GraphSAT(9, 3, 20 / 9, seed=1)
    assert X.M == 20
    levels = {SR.pure_energy(X.A, X.J, s) for s in itertools.product((0, 1), repeat=9)}
    assert len(levels) >= 5
