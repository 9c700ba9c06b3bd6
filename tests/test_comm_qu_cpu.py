"""GraphCommQu without a device: the engine's ΔE formula (csrc/comm_kernels.hpp: from Δ1 / Δ2 alone, no heaps) against the literal
restatement of src/graphs/CommQu.jl (tests/comm_qu_reference.py: ArraySets p2 / m2 and the per-pattern extrema), the refusals that the C ABI
answers before it looks for a device, and the front-end constructors."""
import ctypes as C

import numpy as np
import pytest

import comm_qu_reference as QR

INVALID = 1


def _instance(rng, K1, K2, P, fc):
    N = K1 * K2
    xi = np.tile(rng.integers(0, 2, (P, K1)), (1, K2)) if fc else rng.integers(0, 2, (P, N))
    return xi, rng.integers(0, 2, P), rng.integers(0, 2, N)


@pytest.mark.parametrize("K1,K2,P,fc", [(4, 2, 70, False), (22, 6, 30, True), (2, 4, 129, False)])
def test_formula_equals_the_reference_over_a_random_walk(K1, K2, P, fc):
    """over 2000 flips: the reference's delta_energy over p2 / m2 == the sum over all patterns from the stabilities (and its pruned form) ==
    the difference of the energy's definition; the members of p2 / m2 are the patterns that satisfy the reference's condition, every other
    pattern contributes 0; the stabilities after the walk are a fresh energy()'s"""
    rng = np.random.default_rng(K1 * 1000 + K2 * 100 + P)
    xi, y, s = _instance(rng, K1, K2, P, fc)
    X = QR.make(K2, xi, y)
    E = X.energy(s)
    assert E == QR.energy_from_definition(K2, xi, y, s)
    N = K1 * K2
    nonzero = 0
    for _ in range(2000):
        move = int(rng.integers(0, N))
        d = X.delta(s, move)
        assert d == QR.delta_from_stabilities(X, s, move)
        p2, m2 = X.sets()
        for a in range(P):
            in_p2, in_m2 = X.membership(a)
            assert (a in p2) == in_p2 and (a in m2) == in_m2
            if not in_p2 and not in_m2:
                assert (X._moved(s, move, a) <= 0) == (X.d2[a] <= 0)          # outside both sets: the sign of Δ2 cannot change
        s[move] ^= 1
        assert d == QR.energy_from_definition(K2, xi, y, s) - E
        E += d
        nonzero += d != 0
        X.flip_update(s, move)
    X.check_sets()
    assert nonzero > 0
    fresh = QR.make(K2, xi, y)
    assert fresh.energy(s) == E
    assert X.d1 == fresh.d1 and X.d2 == fresh.d2 and X.sets() == fresh.sets() and X.hmax == fresh.hmax and X.hmin == fresh.hmin


def test_delta2_passes_int16():
    """K1 = 130, K2 = 4: two units on the pattern, two at Hamming distance 65 (Δ1 = 0): Δ2 = ±2 · 130² = ±33 800"""
    K1, K2 = 130, 4
    rng = np.random.default_rng(5)
    xi = rng.integers(0, 2, (2, K1 * K2))
    s = xi[0].copy()
    for u in (2, 3):
        s[u * K1:u * K1 + 65] ^= 1
    X = QR.make(K2, xi, [1, 0])
    X.energy(s)
    assert X.d2[0] == 33800 and [X.d1[u][0] for u in range(4)] == [130, 130, 0, 0]
    X = QR.make(K2, xi, [0, 0])
    X.energy(s)
    assert X.d2[0] == -33800


def test_the_abi_refuses_parity_and_labels_before_it_needs_a_device(pkg):
    L = pkg.lib()
    ctx = C.c_void_p()
    for K1, K2 in ((3, 2), (2, 3), (3, 3), (0, 2), (2, 0)):
        assert L.rrrmc_ctx_create_comm_qu(C.byref(ctx), K1, K2, 1, 0, 0) == INVALID
        assert ctx.value is None
    assert L.rrrmc_ctx_create_comm_qu(C.byref(ctx), 2, 16384, 1, 0, 0) == 3          # N = 32 768: 16-bit Δ1
    assert L.rrrmc_ctx_create_comm_qu(C.byref(ctx), 2, 2, 0, 0, 0) == INVALID        # R < 1
    # under an ensemble and a GraphQuant: Nk = K1 K2 with both even is a multiple of 4
    for create in (L.rrrmc_ctx_create_re, L.rrrmc_ctx_create_le):
        for Nk in (6, 9, 2):
            assert create(C.byref(ctx), Nk, 3, 9, 1, 0, 0) == INVALID
        assert create(C.byref(ctx), 8, 2, 9, 1, 0, 0) == INVALID                     # M must be greater than 2
        assert create(C.byref(ctx), 8, 3, 7, 1, 0, 0) == INVALID                     # kind 7 stays unassigned
        assert create(C.byref(ctx), 8, 3, 10, 1, 0, 0) == INVALID
    assert L.rrrmc_ctx_create_quant_pattern(C.byref(ctx), 9, 12, 3, 3, 1, 0, 0) == INVALID      # K2 odd
    assert L.rrrmc_ctx_create_quant_pattern(C.byref(ctx), 9, 12, 4, 3, 1, 0, 0) == INVALID      # K1 = 3 odd
    assert L.rrrmc_ctx_create_quant_pattern(C.byref(ctx), 7, 12, 2, 3, 1, 0, 0) == INVALID
    assert L.rrrmc_ctx_create_quant_pattern(C.byref(ctx), 8, 12, 2, 3, 1, 0, 0) == INVALID
    assert "rrrmc_ctx_create_comm_qu" in pkg.SYMBOLS
    # the front end refuses the same
    with pytest.raises(ValueError, match="K1 must be even, given: 3"):
        pkg.GraphCommQu(3, 2, 10)
    with pytest.raises(ValueError, match="K2 must be even, given: 3"):
        pkg.GraphCommQu(2, 3, 10)
    with pytest.raises(ValueError, match="a GraphCommQu needs the labels"):
        pkg.GraphCommQu.from_patterns(2, np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError, match="P = 4 labels"):
        pkg.GraphCommQu.from_patterns(2, np.zeros((4, 4), np.int64), np.zeros(5, np.int64))
    with pytest.raises(ValueError, match="not a multiple of K2"):
        pkg.GraphCommQu.from_patterns(4, np.zeros((4, 10), np.int64), np.zeros(4, np.int64))
    with pytest.raises(TypeError):
        pkg.GraphCommQuRE(pkg.GraphCommReLU(2, 2, 4), 3, 1.0, 1.0)                   # a ReLU graph for the Qu alias
    with pytest.raises(TypeError):
        pkg.GraphCommReLULE(pkg.GraphCommQu(2, 2, 4), 3, 1.0, 1.0)
    with pytest.raises(TypeError):
        pkg.GraphQCommQuT(2, 2, 4, 3, 1.0)                                           # neither signature
    with pytest.raises(ValueError, match="greater than 2"):
        pkg.GraphCommQuLE(pkg.GraphCommQu(2, 2, 4), 2, 1.0, 1.0)


@pytest.mark.parametrize("K1,K2,P", [(24, 6, 30), (22, 6, 30), (2, 4, 129)])
def test_front_end_constructors(pkg, K1, K2, P):
    N = K1 * K2
    T = pkg.GraphCommQu(K1, K2, P, seed=11)
    assert (T.N, T.K1, T.K2, T.P, T.K) == (N, K1, K2, P, K2)
    assert pkg.GraphCommQu.model_kind == 36 and pkg.GraphCommQu.energy_dtype == np.int64
    xi, y = T.patterns(), T.labels()
    assert xi.shape == (P, N) and y.shape == (P,) and set(np.unique(xi)) <= {0, 1} and set(np.unique(y)) <= {0, 1}
    # CommQu.gen_ξ (:17-28) is CommReLU's: the same draw
    R = pkg.GraphCommReLU(K1, K2, P, seed=11)
    assert (T.xi == R.xi).all() and (T.y == R.y).all()
    assert (pkg.GraphCommQu(K1, K2, P, seed=12).xi != T.xi).any()
    F = pkg.GraphCommQu(K1, K2, P, fc=True, seed=11)
    fx = F.patterns()
    for k in range(K2):                                                   # fc: the K1 columns repeated K2 times (:93-96)
        assert (fx[:, k * K1:(k + 1) * K1] == fx[:, :K1]).all()
    assert any((xi[:, k * K1:(k + 1) * K1] != xi[:, :K1]).any() for k in range(1, K2))
    Y = pkg.GraphCommQu.from_patterns(K2, fx, F.labels())
    assert (Y.xi == F.xi).all() and (Y.y == F.y).all() and (Y.K1, Y.K2, Y.N, Y.P) == (K1, K2, N, P)
    if N % 64:
        assert not (T.xi[:, -1] >> np.uint64(N % 64)).any()
    if P % 64:
        assert not (T.y[-1] >> np.uint64(P % 64)).any()
    # the aliases: both signatures, the slice kind and the selectors of rrrmc_ctx_create_multi
    for ens, model, sites in ((pkg.GraphCommQuRE, 37, N * 5), (pkg.GraphCommQuLE, 38, N * 6)):
        a, b = ens(T, 5, 0.5, 2.0), ens(K1, K2, P, 5, 0.5, 2.0, seed=11)
        assert a.X1 is T and (b.X1.xi == T.xi).all() and (b.X1.y == T.y).all()
        assert a.slice_kind == b.slice_kind == 9 and a.model_kind == b.model_kind == model and a.Nk == N and a.M == 5 and a.N == sites
        assert (ens(K1, K2, P, 5, 0.5, 2.0, fc=True, seed=11).X1.xi == F.xi).all()
    Q = pkg.GraphQCommQuT(K1, K2, P, 5, 0.5, 2.0, seed=11)
    assert Q.pat_slices == 9 and Q._multi_args() == (39, N, K2, 5) and (Q.X1.xi == T.xi).all() and Q.N == 5 * N
    assert pkg.GraphQCommQuT(T, 5, 0.5, 2.0).X1 is T
    import quant_pattern_reference as QP
    assert Q.fourK == QP.quant_fourK(2.0, 0.5, 5)
