"""CPU checks of the regular 3-spin model (src/graphs/PSpin3.jl).  The first test validates the MODEL the engine is built on, inside
tests/pspin3_reference.py alone: ΔE written as a function of the configuration (what csrc/pspin_core.hpp computes, 2 (2c − K)) equals the
literal LocalFields{Int} cache restated from the reference after random accepted and undone moves, and the tracked energy equals
−Σ_triples σσσ — no library code runs in it (the library's own pspin_delta is held to a direct sum by tests/pspin_core_check.cpp, and to
the literal cache by the GPU parity tests).  The others run library code: the host generator's tables are partitions named by the seed;
every refusal that needs no device returns its code; the front end carries the reference's attributes."""
import ctypes as C

import numpy as np
import pytest

import pspin3_reference as PR

SHAPES = [(3, 1), (3, 2), (6, 3), (33, 4), (96, 5), (192, 16)]


def _doubled_layer_instance():
    """N = 9, K = 3: layer 0 given twice (every pair of it counts twice), then another partition"""
    l0 = [(0, 1, 2), (3, 4, 5), (6, 7, 8)]
    l1 = [(0, 3, 6), (1, 4, 7), (2, 5, 8)]
    return 9, [l0, l0, l1]


def _tables(pkg):
    for N, K in SHAPES:
        yield N, np.asarray(pkg.GraphPSpin3(N, K, seed=1000 + N).A)
    N, layers = _doubled_layer_instance()
    yield N, PR.table_from_triples(N, layers)


def test_pure_delta_equals_the_literal_cache_over_accepted_and_undone_moves(pkg):
    for N, A in _tables(pkg):
        K = A.shape[1] // 2
        X = PR.PSpin3Ref(N, A)
        rng = np.random.default_rng(N + K)
        s = rng.integers(0, 2, N)
        E = X.energy(s)
        assert E == PR.pure_energy(A, s)
        seen = set()
        for step in range(1500):
            i = int(rng.integers(N))
            d = X.delta_energy(i)
            c = sum(int(s[i]) ^ int(s[A[i, 2 * k]]) ^ int(s[A[i, 2 * k + 1]]) for k in range(K))
            assert d == PR.pure_delta(A, s, i) == 2 * (2 * c - K)
            seen.add(abs(d))
            s[i] ^= 1
            X.update_cache(s, i)
            if step % 3 == 1:                                          # an undone move: the swap path over U (PSpin3.jl:102-111)
                assert X.move_last == i
                s[i] ^= 1
                X.update_cache(s, i)
                assert X.delta_energy(i) == d
            else:
                E += d
            assert E == PR.pure_energy(A, s)                           # E tracked by ΔE equals the energy of the definition
            assert all(X.delta_energy(j) == PR.pure_delta(A, s, j) for j in X.U[i] + [i])
        assert [X.delta_energy(j) for j in range(N)] == [PR.pure_delta(A, s, j) for j in range(N)]
        Y = PR.PSpin3Ref(N, A)                                         # the walked cache equals a fresh one
        assert Y.energy(s) == E and Y.lfields == X.lfields
        assert seen <= set(PR.all_delta_e(K))


def test_all_delta_e(pkg):
    assert PR.all_delta_e(1) == (2,) and PR.all_delta_e(2) == (0, 4) and PR.all_delta_e(3) == (2, 6) and PR.all_delta_e(4) == (0, 4, 8)
    for N, K in SHAPES:
        X = pkg.GraphPSpin3(N, K, seed=3)
        assert pkg.all_delta_e(X) == PR.all_delta_e(K)
        # every value a configuration can give is in the table, and the extremes are reached
        assert {abs(2 * (2 * c - K)) for c in range(K + 1)} == set(PR.all_delta_e(K))


@pytest.mark.parametrize("N,K", SHAPES + [(999, 7)])
def test_generator_every_layer_a_partition_and_named_by_the_seed(pkg, N, K):
    L = pkg.lib()
    A = np.full((N, 2 * K), -1, np.int32)
    assert L.rrrmc_gen_pspin3(N, K, 77, A.reshape(-1)) == 0
    layers = PR.layers_of(A)                                           # raises unless every layer partitions the sites into triples
    assert len(layers) == K
    for i in range(N):                                                 # the triple's own order: v1 lists (v2, v3), v2 (v1, v3), v3 (v1, v2)
        for k in range(K):
            y, z = int(A[i, 2 * k]), int(A[i, 2 * k + 1])
            assert {int(A[y, 2 * k]), int(A[y, 2 * k + 1])} == {i, z} and {int(A[z, 2 * k]), int(A[z, 2 * k + 1])} == {i, y}
    B = np.zeros_like(A)
    assert L.rrrmc_gen_pspin3(N, K, 77, B.reshape(-1)) == 0 and (A == B).all()
    assert (pkg.GraphPSpin3(N, K, seed=77).A == A).all()
    if N > 3:
        assert L.rrrmc_gen_pspin3(N, K, 78, B.reshape(-1)) == 0 and (A != B).any()
    if N > 3 and K > 1:
        assert layers[0] != layers[1]                                  # the layers are drawn independently


def test_every_refusal_that_needs_no_device_returns_its_code(pkg):
    L = pkg.lib()
    INVALID, UNSUPPORTED = 1, 3
    buf = np.zeros(65538 * 2, np.int32)
    assert L.rrrmc_gen_pspin3(6, 1, 1, None) == INVALID
    assert L.rrrmc_gen_pspin3(0, 1, 1, buf) == INVALID
    for N, K in ((4, 1), (5, 3), (65538, 1), (6, 17), (6, 0)):         # N % 3 != 0, N > 65 535, K outside 1 .. 16
        assert L.rrrmc_gen_pspin3(N, K, 1, buf) == UNSUPPORTED, (N, K)
    assert L.rrrmc_gen_pspin3(65535, 1, 1, buf) == 0 and L.rrrmc_gen_pspin3(6, 16, 1, buf) == 0
    ctx = C.c_void_p()
    for wrap in (0, 1, 2):                                             # the creator checks its arguments before it asks for a device
        for N, K in ((4, 1), (65538, 1), (6, 17), (6, 0)):
            assert L.rrrmc_ctx_create_pspin3(C.byref(ctx), N, K, wrap, 1, 0, 0) == UNSUPPORTED and not ctx.value
            assert str(N if N != 6 else K) in L.rrrmc_last_error(None).decode()
        assert L.rrrmc_ctx_create_pspin3(C.byref(ctx), 6, 3, wrap, 0, 0, 0) == INVALID
        assert L.rrrmc_ctx_create_pspin3(C.byref(ctx), 6, 3, wrap, 1, 0, 5) == INVALID          # replica0 % 32
    assert L.rrrmc_ctx_create_pspin3(C.byref(ctx), 6, 3, 3, 1, 0, 0) == INVALID and L.rrrmc_ctx_create_pspin3(C.byref(ctx), 6, 3, -1, 1, 0, 0) == INVALID
    assert L.rrrmc_ctx_create_pspin3(None, 6, 3, 0, 1, 0, 0) == INVALID
    # the other creators keep refusing the new slice kind and the new models
    assert L.rrrmc_ctx_create_af(C.byref(ctx), 14, 0, 6, 0, 1, 0, 0) == INVALID
    for create in (L.rrrmc_ctx_create_re, L.rrrmc_ctx_create_le, L.rrrmc_ctx_create_tle):
        assert create(C.byref(ctx), 6, 3, 14, 1, 0, 0) != 0
    assert L.rrrmc_ctx_create_mixed(C.byref(ctx), np.array([14, 0], np.int32), 2, 0, 6, 0, 0, 1, 0, 0) != 0
    # the front end
    for N, K in ((4, 1), (0, 1), (6, 0)):
        with pytest.raises(ValueError):
            pkg.GraphPSpin3(N, K)
    with pytest.raises(pkg.RRRMCError) as e:
        pkg.GraphPSpin3(6, 17)
    assert e.value.code == UNSUPPORTED
    good = [(0, 1, 2), (3, 4, 5)]
    for layers in ([], [[(0, 1, 2)]], [[(0, 1, 2), (3, 4, 6)]], [[(0, 1, 2), (2, 4, 5)]], [good, [(0, 1, 2), (3, 4, -1)]], [[(0, 1), (2, 3), (4, 5)]]):
        with pytest.raises(ValueError):
            pkg.GraphPSpin3.from_triples(6, layers)
    with pytest.raises(ValueError):
        pkg.GraphPSpin3.from_triples(7, [good])


def test_front_end_attributes_and_refusals(pkg):
    N, layers = _doubled_layer_instance()
    X = pkg.GraphPSpin3.from_triples(N, layers)
    R = PR.PSpin3Ref(N, PR.table_from_triples(N, layers))
    assert (X.N, X.K) == (9, 3) and X.A.tolist() == R.A and X.A.dtype == np.int32
    assert X.model_kind == 105 and X.energy_dtype == np.int64 and pkg.getN(X) == 9
    for i in range(N):
        assert pkg.neighbors(X, i).tolist() == R.U[i]                  # unique(A[i]) in first-occurrence order
    assert pkg.neighbors(X, 0).tolist() == [1, 2, 3, 6] and X.A[4].tolist() == [3, 5, 3, 5, 1, 7]
    assert pkg.all_delta_e(X) == (2, 6)
    h = np.linspace(-1.0, 1.0, N)
    a, s = pkg.GraphAddFields(h, X), pkg.GraphAddSubFields(h, X)
    assert (a.model_kind, s.model_kind) == (106, 107) and a.slice_kind == s.slice_kind == 14 and a.X1 is X
    assert a._multi_args() == (106, 9, 3, 0) and s._multi_args() == (107, 9, 3, 0) and X._multi_args() == (105, 9, 3, 0)
    with pytest.raises(ValueError):
        pkg.GraphAddFields(h[:-1], X)
    for make in (lambda: pkg.GraphMixed(X, None), lambda: pkg.GraphMixed(pkg.GraphSK(9, seed=1), X), lambda: pkg.GraphQuant(X, 3, 0.5, 1.0),
                 lambda: pkg.GraphRobustEnsemble(9, 3, 1.0, 1.0, X), lambda: pkg.GraphLocalEntropy(9, 3, 1.0, 1.0, X),
                 lambda: pkg.GraphTopologicalLocalEntropy(9, 3, 1.0, 0.5, 1.0, X)):
        with pytest.raises(TypeError) as e:
            make()
        assert "GraphPSpin3" in str(e.value) and "GraphAddFields" in str(e.value)
    for name in ("rrrmc_ctx_create_pspin3", "rrrmc_set_pspin3", "rrrmc_pspin_build", "rrrmc_gen_pspin3"):
        assert name in pkg.SYMBOLS
