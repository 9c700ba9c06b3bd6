"""CPU checks of the binary perceptron graphs (src/graphs/PercStep.jl, PercLinear.jl): the restatement (tests/perc_reference.py) satisfies
the reference's own check_delta invariant, the engine's P-bit masks are the reference's ArraySets over any walk of flips, the constructors
refuse what the reference refuses, and the pattern packing is loss-free."""
import numpy as np
import pytest

import perc_reference as PR


def _patterns(rng, P, N):
    return rng.integers(0, 2, (P, N))


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("N,P", [(101, 30), (1, 1), (3, 2), (7, 65), (33, 64), (65, 129)])
def test_check_delta_holds_for_every_site(linear, N, P):
    # check_delta (PercStep.jl:175-183, PercLinear.jl:179-187): delta_energy == energy(flipped) - energy.  GraphPercStep: integers, exact.
    # GraphPercLinear: both energies are 2 n / sqrt(N) of integers n, so the invariant is asserted exactly on the numerators (delta_energy is
    # 2 (n1 - n0) / sqrt(N), the Float64 the reference returns) and within the rounding of one subtraction on the Float64 difference
    rng = np.random.default_rng(1000 * N + P + linear)
    xi = _patterns(rng, P, N)
    X = PR.make(xi, linear)
    for _ in range(3):
        s = rng.integers(0, 2, N)
        e0 = X.energy(s)
        deltas = [X.delta(s, i) for i in range(N)]
        for i in range(N):
            s[i] ^= 1
            e1 = PR.make(xi, linear).energy(s)
            s[i] ^= 1
            if linear:
                n = round((e1 - e0) * X.sN / 2)
                assert deltas[i] == 2 * n / X.sN
                assert abs((e1 - e0) - deltas[i]) <= 4 * np.spacing(max(abs(e0), abs(e1), 1.0))
            else:
                assert deltas[i] == e1 - e0


@pytest.mark.parametrize("linear", [False, True])
def test_masks_equal_arraysets_over_a_random_walk(linear):
    # the kernels keep p and m as masks computed from Δ alone (csrc/perc_kernels.hpp); the reference keeps ArraySets through push! / delete!
    rng = np.random.default_rng(7 + linear)
    N, P = 9, 70                                   # small N: the stabilities cross ±1 all the time
    xi = _patterns(rng, P, N)
    X = PR.make(xi, linear)
    s = rng.integers(0, 2, N)
    X.energy(s)
    assert X.members() == PR.masks_of(X.ds, linear)
    for _ in range(2000):
        i = int(rng.integers(N))
        d = X.delta(s, i)
        p, m = PR.masks_of(X.ds, linear)
        col = xi[:, i] ^ s[i]
        dm = sum(1 - col[a] for a in p) - sum(col[a] for a in m) + (sum(1 - col[a] for a in m) if linear else 0)
        assert d == (2 * int(dm) / X.sN if linear else dm)
        s[i] ^= 1
        X.flip_update(s, i)
        X.p.check()
        X.m.check()
        assert X.members() == PR.masks_of(X.ds, linear)
        assert X.ds == [N - 2 * int((s ^ xi[a]).sum()) for a in range(P)]
    # and a flip followed by its undo restores everything (what lets rrrMC update a slice only for accepted moves)
    before = (list(X.ds), X.members())
    s[3] ^= 1
    X.flip_update(s, 3)
    s[3] ^= 1
    X.flip_update(s, 3)
    assert (list(X.ds), X.members()) == before


def test_constructors_refuse_bad_input(pkg):
    for G in (pkg.GraphPercStep, pkg.GraphPercLinear):
        with pytest.raises(ValueError, match="N must be odd"):
            G(100, 30)
        with pytest.raises(ValueError):
            G(101, 0)
        with pytest.raises(ValueError, match="N must be odd"):
            G.from_patterns(np.zeros((3, 4), np.int64))
        with pytest.raises(ValueError, match="P x N"):
            G.from_patterns(np.zeros(5, np.int64))
        with pytest.raises(ValueError, match="P x N"):
            G.from_patterns(np.zeros((2, 3, 5), np.int64))
        with pytest.raises(ValueError, match="0/1"):
            G.from_patterns(np.full((2, 3), 2))
    X = pkg.GraphPercStep(11, 4)
    with pytest.raises(TypeError):
        pkg.GraphPercLinearRE(X, 3, 1.0, 1.0)                      # a step graph for the linear alias
    with pytest.raises(TypeError):
        pkg.GraphPercStepRE(11, 4, 3, 1.0)                         # neither signature
    with pytest.raises(ValueError, match="greater than 2"):
        pkg.GraphPercStepLE(X, 2, 1.0, 1.0)
    with pytest.raises(ValueError):
        pkg.graphs.unpack_patterns(np.zeros((4, 3), np.uint64), 11)       # wrong number of chunks


def test_ensemble_constructors_share_one_pattern_matrix(pkg):
    X = pkg.GraphPercLinear(21, 9, seed=5)
    for ens, kind, model in ((pkg.GraphPercLinearRE, 4, 20), (pkg.GraphPercLinearLE, 4, 22)):
        a, b = ens(X, 5, 0.5, 2.0), ens(21, 9, 5, 0.5, 2.0, seed=5)
        assert a.X1 is X and (b.X1.xi == X.xi).all()
        assert a.slice_kind == b.slice_kind == kind and a.model_kind == b.model_kind == model
        assert a.Nk == 21 and a.M == 5
    assert pkg.GraphPercStepRE(21, 9, 5, 0.5, 2.0).model_kind == 19 and pkg.GraphPercStepLE(21, 9, 5, 0.5, 2.0).model_kind == 21
    assert pkg.GraphPercStep.energy_dtype == np.int64 and pkg.GraphPercLinear.energy_dtype == np.float64


@pytest.mark.parametrize("N,P", [(101, 30), (63, 1), (65, 64), (129, 130)])
def test_pattern_packing_round_trip(pkg, N, P):
    rng = np.random.default_rng(N + P)
    xi = rng.integers(0, 2, (P, N))
    X = pkg.GraphPercStep.from_patterns(xi)
    assert X.xi.shape == (P, (N + 63) // 64) and X.xi.dtype == np.uint64
    assert (X.patterns() == xi).all()
    if N % 64:
        assert not (X.xi[:, -1] >> np.uint64(N % 64)).any()       # no bits beyond N
    Y = pkg.GraphPercLinear(N, P, seed=3)
    assert (pkg.graphs.pack_patterns(Y.patterns()) == Y.xi).all()
    assert (pkg.GraphPercLinear(N, P, seed=3).xi == Y.xi).all() and (pkg.GraphPercLinear(N, P, seed=4).xi != Y.xi).any()
    if N % 64:
        assert not (Y.xi[:, -1] >> np.uint64(N % 64)).any()
