"""CPU checks for the ensembles over sparse Float64 slices (GraphEARE, GraphEALE, GraphEATLE; no device is touched).

1. The slice restatement (tests/sparse_slice_reference.py, from EA.jl:584-680) against brute force: after every one of a few hundred random
   flips and flip-backs, delta(s, i) equals E(flip) - E recomputed from the definition (exact sums, math.fsum) to within the rounding of
   K + 1 additions, stated as 8 K max|J| 2^-52 (the bound does not grow with the number of updates made so far); the undo path restores
   lfields bit for bit; and at the end every cached field is within the same bound of the field of a freshly built cache.  On EA(L=2, D=2), where every neighbour appears twice, and on EA(L=3, D=2).
2. The front-end objects: sizes, model and slice kinds, the TLE topology uA, the seeded alias, the refusals made before any device call."""
import random

import numpy as np
import pytest

import sparse_slice_reference as SP


def _lattice(pkg, L, D, seed):
    X = pkg.GraphEARE(L, D, 3, 1.0, 1.0, seed=seed).X1
    return X.A, X.J


@pytest.mark.parametrize("L,D", [(2, 2), (3, 2)])
def test_slice_delta_is_the_energy_difference_and_undo_is_exact(pkg, L, D):
    A, J = _lattice(pkg, L, D, 1234 + L)
    Nk, K = A.shape
    bound = 8 * K * float(np.abs(J).max()) * 2.0 ** -52
    rng = random.Random(99 + L)
    s = np.array([rng.randrange(2) for _ in range(Nk)], np.int64)
    X = SP.SliceSparseF64(A, J)
    E = X.energy(s)
    assert abs(E - SP.brute_energy(A, J, s)) <= bound * Nk          # energy() adds Nk such sums
    if L == 2:
        assert all(len(u) == D for u in X.uA) and all(len(a) == 2 * D for a in X.A)          # every neighbour twice
    for step in range(300):
        i = rng.randrange(Nk)
        E0 = SP.brute_energy(A, J, s)
        s2 = s.copy()
        s2[i] ^= 1
        dE = SP.brute_energy(A, J, s2) - E0
        assert abs(X.delta(s, i) - dE) <= bound, (step, i)
        before = list(X.lf)
        s[i] ^= 1
        X.flip_update(s, i)
        assert X.move_last == i
        if rng.random() < 0.5:                   # flip back at once: the move_last path, the exact undo of a rejected move
            s[i] ^= 1
            X.flip_update(s, i)
            assert X.lf == before, (step, i)     # bit for bit (== on floats; no NaN here)
            assert X.move_last == i
            if rng.random() < 0.3:               # forth and back again: the record is swapped both ways
                s[i] ^= 1
                X.flip_update(s, i)
                s[i] ^= 1
                X.flip_update(s, i)
                assert X.lf == before, (step, i)
    # the cache still describes the configuration
    Y = SP.SliceSparseF64(A, J)
    Y.energy(s)
    assert max(abs(a - b) for a, b in zip(X.lf, Y.lf)) <= bound


def test_a_doubled_bond_is_applied_twice_in_row_order():
    # two sites joined by two bonds of different strength (the L = 2 case of one dimension): J values whose sum rounds differently by order
    A = np.array([[1, 1], [0, 0]], np.int32)
    J = np.array([[1.0, 2.0 ** -53], [1.0, 2.0 ** -53]])
    X = SP.SliceSparseF64(A, J)
    s = np.array([1, 1], np.int64)
    assert X.energy(s) == -(1.0 + 2.0 ** -53) and X.uA == [[1], [0]]
    lf0 = list(X.lf)
    s[0] ^= 1
    X.flip_update(s, 0)
    want = lf0[1]
    want -= 4 * -1 * 1.0
    want -= 4 * -1 * 2.0 ** -53
    assert X.lf[1] == want and X.lf[0] == -lf0[0]
    s[0] ^= 1
    X.flip_update(s, 0)
    assert X.lf == lf0


@pytest.mark.parametrize("L,D,M", [(2, 2, 3), (3, 2, 4), (3, 3, 5)])
def test_front_end_objects(pkg, L, D, M):
    Nk, K = L ** D, 2 * D
    Xre = pkg.GraphEARE(L, D, M, 1.5, 2.0, seed=5)
    Xle = pkg.GraphEALE(L, D, M, 1.5, 2.0, seed=5)
    Xtle = pkg.GraphEATLE(L, D, M, 1.5, 0.3, 2.0, seed=5)
    assert (Xre.Nk, Xre.N, Xre.K, Xre.model_kind, Xre.slice_kind) == (Nk, Nk * M, K, 67, 12)
    assert (Xle.Nk, Xle.N, Xle.K, Xle.model_kind, Xle.slice_kind) == (Nk, Nk * (M + 1), K, 68, 12)
    assert (Xtle.Nk, Xtle.N, Xtle.K, Xtle.model_kind, Xtle.slice_kind) == (Nk, Nk * (M + 1), K, 69, 12)
    assert Xre._multi_args() == (67, Nk, K, M) and Xle._multi_args() == (68, Nk, K, M) and Xtle._multi_args() == (69, Nk, K, M)
    # one shared (A, J), the same for the same seed
    assert (Xre.X1.A == Xle.X1.A).all() and (Xre.X1.J == Xle.X1.J).all() and (Xre.X1.J == Xtle.X1.J).all()
    assert (pkg.GraphEARE(L, D, M, 1.5, 2.0, seed=6).X1.J != Xre.X1.J).any()
    A, J = Xre.X1.A, Xre.X1.J
    assert A.shape == J.shape == (Nk, K) and isinstance(Xre.X1, pkg.GraphEANormal)
    # J = 4u - 2 in [-2, 2), every bond from both ends with one value
    assert (J >= -2.0).all() and (J < 2.0).all() and len(np.unique(J)) == Nk * K // 2
    for x in range(Nk):
        for y in set(A[x].tolist()):
            assert sorted(J[x][A[x] == y].tolist()) == sorted(J[y][A[y] == x].tolist())
    # the TLE topology is uA: the distinct entries of the row, ascending
    ref = SP.SliceSparseF64(A, J)
    assert Xtle.neighb == ref.uA == [sorted(set(A[x].tolist())) for x in range(Nk)]
    assert Xtle.max_deg == (D if L == 2 else 2 * D)
    assert Xtle._rowptr.tolist() == [len(ref.uA[0]) * x for x in range(Nk + 1)]
    # the X forms keep X.A, X.J
    X1 = Xre.X1
    assert pkg.GraphEALE(X1, M, 1.0, 1.0).X1 is X1 and pkg.GraphEATLE(X1, M, 1.0, 0.5, 1.0).X1 is X1 and pkg.GraphEARE(X1, M, 1.0, 1.0).X1 is X1


def test_generic_constructors_take_a_rrg_normal(pkg):
    G = pkg.GraphRRGNormal(10, 3, seed=4)
    Xre = pkg.GraphRobustEnsemble(10, 4, 1.0, 1.0, G)
    Xle = pkg.GraphLocalEntropy(10, 4, 1.0, 1.0, G)
    Xtle = pkg.GraphTopologicalLocalEntropy(10, 4, 1.0, 0.5, 1.0, G)
    assert (Xre.model_kind, Xle.model_kind, Xtle.model_kind) == (67, 68, 69)
    assert Xre.K == Xle.K == Xtle.K == 3 and Xre.slice_kind == 12
    assert Xtle.neighb == [sorted(set(G.A[x].tolist())) for x in range(10)]


def test_the_uniform_generator(pkg):
    L = pkg.lib()
    A = np.zeros((9, 4), np.int32)
    assert L.rrrmc_gen_ea(3, 2, A) == 0
    J1, J2, J3 = np.zeros((9, 4)), np.zeros((9, 4)), np.zeros((9, 4))
    assert L.rrrmc_gen_couplings_uniform(9, 4, A, 7, -2.0, 2.0, J1.reshape(-1)) == 0
    assert L.rrrmc_gen_couplings_uniform(9, 4, A, 7, 0.0, 1.0, J2.reshape(-1)) == 0
    assert L.rrrmc_gen_couplings_uniform(9, 4, A, 8, -2.0, 2.0, J3.reshape(-1)) == 0
    assert (J2 >= 0).all() and (J2 < 1).all() and (J1 == -2.0 + 4.0 * J2).all() and (J1 != J3).any()
    # the bond visiting order of gen_J: x < y in (x, k) order takes draw 0, 1, ...; the gauss generator visits the same slots
    G = np.zeros((9, 4))
    assert L.rrrmc_gen_couplings_gauss(9, 4, A, 7, G.reshape(-1)) == 0
    first = lambda M: [M[x, k] for x in range(9) for k in range(4) if x < A[x, k]]
    assert len(set(first(J2))) == 18 and [np.argwhere(J2 == v).tolist() for v in first(J2)] == [np.argwhere(G == v).tolist() for v in first(G)]
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf"))):
        assert L.rrrmc_gen_couplings_uniform(9, 4, A, 7, lo, hi, J1.reshape(-1)) == 1


def test_bad_slice_graphs_are_refused_before_any_device_call(pkg):
    good = pkg.GraphEARE(3, 2, 3, 1.0, 1.0, seed=1).X1
    odd = pkg.GraphEANormal.from_AJ(good.A[:, :3].copy(), good.J[:, :3].copy())
    for make in (lambda X: pkg.GraphEARE(X, 3, 1.0, 1.0), lambda X: pkg.GraphEALE(X, 3, 1.0, 1.0), lambda X: pkg.GraphEATLE(X, 3, 1.0, 0.5, 1.0)):
        with pytest.raises(ValueError, match="twoD must be even, given: 3"):
            make(odd)
        A = good.A.copy()
        A[4] = A[4][::-1]
        with pytest.raises(ValueError, match="row 5 is not sorted"):
            make(pkg.GraphEANormal.from_AJ(A, good.J))
        A = good.A.copy()
        A[2, 0] = 2
        with pytest.raises(ValueError):
            make(pkg.GraphEANormal.from_AJ(np.sort(A, axis=1), good.J))
        Jn = good.J.copy()
        Jn[0, 0] = np.inf
        with pytest.raises(ValueError, match="finite"):
            make(pkg.GraphEANormal.from_AJ(good.A, Jn))
    with pytest.raises(ValueError, match="M must be greater than 2"):
        pkg.GraphEARE(3, 2, 2, 1.0, 1.0)
    with pytest.raises(ValueError, match="D must be"):
        pkg.GraphEATLE(3, 0, 3, 1.0, 0.5, 1.0)
    with pytest.raises(ValueError, match="expected Nk = 7"):
        pkg.GraphRobustEnsemble(7, 3, 1.0, 1.0, good)
    # L = 1: every site is its own neighbour
    with pytest.raises((ValueError, pkg.RRRMCError)):
        pkg.GraphEATLE(1, 2, 3, 1.0, 0.5, 1.0)


def test_reference_objects_agree_with_their_definitions():
    # the helpers that wrap the slice into the RE / LE / TLE restatements: energies are the inner graph's plus the slices'
    rng = random.Random(5)
    A = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    J = np.array([[0.5, -1.25], [0.5, 0.75], [-1.25, 0.75]])
    M = 3
    for make, rows in ((lambda: SP.make_re(A, J, M, 1.5, 2.0), M), (lambda: SP.make_le(A, J, M, 1.5, 2.0), M + 1),
                       (lambda: SP.make_tle(A, J, M, 1.5, 0.25, 2.0), M + 1)):
        X = make()
        s = np.array([rng.randrange(2) for _ in range(3 * rows)], np.int64)
        E = X.energy(s)
        for move in range(3 * rows):
            X2 = make()
            s2 = s.copy()
            s2[move] ^= 1
            d = (X.lf0[move] + X.residual(move)) if rows == M else X.delta(move)
            assert abs((X2.energy(s2) - E) - d) < 1e-12
    assert SP.make_tle(A, J, M, 1.0, 1.0, 1.0).neighb == [[1, 2], [0, 2], [0, 1]]
