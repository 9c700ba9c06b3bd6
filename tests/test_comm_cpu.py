"""CPU checks of the binary committee machines (src/graphs/CommStep.jl, CommReLU.jl): the restatement (tests/comm_reference.py) satisfies
the reference's check_delta invariant at every site, the engine's popcount form of delta_energy and its P-bit masks equal the reference's
ArraySets over any walk of flips, pattern generation (tree and fc) and packing are loss-free and seeded, and the constructors refuse what the
reference refuses."""
import numpy as np
import pytest

import comm_reference as CR

SHAPES = [  # (K1, K2, P, fc): K2 = 1, P < 64, P = 64, P > 64
    (5, 3, 30, False), (5, 3, 30, True), (7, 1, 64, False), (3, 5, 129, True), (9, 3, 65, False)]
RELU_SHAPES = [(4, 2, 30, False), (4, 2, 30, True), (6, 2, 64, False), (2, 4, 129, True), (4, 4, 65, False), (8, 2, 7, False)]


def _instance(rng, K1, K2, P, fc, relu):
    Kin = K1 if fc else K1 * K2
    xi = np.tile(rng.integers(0, 2, (P, Kin)), (1, K2 if fc else 1))
    y = rng.integers(0, 2, P) if relu else None
    return xi, y


@pytest.mark.parametrize("relu,K1,K2,P,fc", [(False,) + s for s in SHAPES] + [(True,) + s for s in RELU_SHAPES])
def test_delta_energy_equals_the_energy_difference_at_every_site(relu, K1, K2, P, fc):
    # check_delta (CommStep.jl:244-252, CommReLU.jl:268-276): delta_energy == energy(flipped) - energy, integers, exact; and the engine's
    # popcount rows over masks give the same number
    rng = np.random.default_rng(1000 * K1 + 10 * K2 + P + 7 * relu + fc)
    for _ in range(4):
        xi, y = _instance(rng, K1, K2, P, fc, relu)
        X = CR.make(K2, xi, y)
        s = rng.integers(0, 2, K1 * K2)
        e0 = X.energy(s)
        assert e0 == CR.energy_from_definition(K2, xi, y, s)
        for i in range(K1 * K2):
            d = X.delta(s, i)
            assert d == CR.delta_from_masks(X, s, i)
            s[i] ^= 1
            e1 = CR.make(K2, xi, y).energy(s)
            s[i] ^= 1
            assert d == e1 - e0, (i, d, e1, e0)


@pytest.mark.parametrize("relu,K1,K2,P", [(False, 3, 3, 70), (False, 5, 1, 40), (True, 2, 4, 70), (True, 4, 2, 130)])
def test_masks_equal_arraysets_over_a_random_walk(relu, K1, K2, P):
    # the kernels keep p1, m1, p2, m2 as masks computed from Δ1 / Δ2 alone; the reference keeps ArraySets through push! / delete!
    rng = np.random.default_rng(17 + K1 + 10 * relu)
    N = K1 * K2
    xi, y = _instance(rng, K1, K2, P, False, relu)
    X = CR.make(K2, xi, y)
    s = rng.integers(0, 2, N)
    s0 = s.copy()
    X.energy(s)
    assert X.sets() == CR.masks_of(X)
    walk = []
    for _ in range(1500):
        i = int(rng.integers(N))
        assert X.delta(s, i) == CR.delta_from_masks(X, s, i)
        s[i] ^= 1
        X.flip_update(s, i)
        walk.append(i)
        X.check_sets()
        assert X.sets() == CR.masks_of(X)
        fresh = CR.make(K2, xi, y)
        fresh.energy(s)
        assert X.d1 == fresh.d1 and X.d2 == fresh.d2
    for i in reversed(walk):                       # flip-backs: the walk ends where it started, with the start's state
        s[i] ^= 1
        X.flip_update(s, i)
        assert X.sets() == CR.masks_of(X)
    assert (s == s0).all()
    fresh = CR.make(K2, xi, y)
    fresh.energy(s)
    assert X.d1 == fresh.d1 and X.d2 == fresh.d2 and X.sets() == CR.masks_of(fresh)


@pytest.mark.parametrize("relu,K1,K2,P", [(False, 21, 5, 30), (False, 3, 1, 64), (True, 22, 6, 30), (True, 24, 6, 130)])
def test_generation_fc_seeds_and_packing(pkg, relu, K1, K2, P):
    G = pkg.GraphCommReLU if relu else pkg.GraphCommStep
    N = K1 * K2
    X = G(K1, K2, P, fc=True, seed=11)
    xi = X.patterns()
    assert xi.shape == (P, N)
    for k in range(K2):                                                   # the K1 columns repeated K2 times
        assert (xi[:, k * K1:(k + 1) * K1] == xi[:, :K1]).all()
    T = G(K1, K2, P, seed=11)
    assert (G(K1, K2, P, seed=11).xi == T.xi).all() and (G(K1, K2, P, seed=12).xi != T.xi).any()
    if K2 > 1:
        assert any((T.patterns()[:, k * K1:(k + 1) * K1] != T.patterns()[:, :K1]).any() for k in range(1, K2))
    # the tree draw of Kin = N bits is rrrmc_gen_patterns' draw of N bits, so K2 = 1 is the perceptron's matrix
    if not relu and K2 == 1:
        assert (T.xi == pkg.GraphPercStep(N, P, seed=11).xi).all()
    if relu:
        y = T.labels()
        assert y.shape == (P,) and set(np.unique(y)) <= {0, 1}
        assert (G(K1, K2, P, seed=11).labels() == y).all() and (G(K1, K2, P, seed=12).labels() != y).any()
        assert not (T.y[-1] >> np.uint64(P % 64)).any() if P % 64 else True        # no label bits beyond P
    else:
        assert T.y is None and T.labels() is None
    Y = G.from_patterns(K2, xi, X.labels())
    assert (Y.xi == X.xi).all() and (Y.patterns() == xi).all()
    if relu:
        assert (Y.y == X.y).all() and (Y.labels() == X.labels()).all()
    if N % 64:
        assert not (X.xi[:, -1] >> np.uint64(N % 64)).any() and not (T.xi[:, -1] >> np.uint64(N % 64)).any()       # no bits beyond N
    assert X.K1 == K1 and X.K2 == K2 and X.N == N and X.P == P


def test_constructors_refuse_bad_input(pkg):
    with pytest.raises(ValueError, match="K1 must be odd, given: 4"):
        pkg.GraphCommStep(4, 3, 10)
    with pytest.raises(ValueError, match="K2 must be odd, given: 2"):
        pkg.GraphCommStep(3, 2, 10)
    with pytest.raises(ValueError, match="K1 must be even, given: 3"):
        pkg.GraphCommReLU(3, 2, 10)
    with pytest.raises(ValueError, match="K2 must be even, given: 3"):
        pkg.GraphCommReLU(2, 3, 10)
    with pytest.raises(ValueError, match="not a multiple of K2"):
        pkg.GraphCommStep.from_patterns(3, np.zeros((4, 10), np.int64))            # N % K2 != 0
    with pytest.raises(ValueError, match="K1 must be odd, given: 2"):
        pkg.GraphCommStep.from_patterns(3, np.zeros((4, 6), np.int64))
    with pytest.raises(ValueError, match="K2 must be even, given: 1"):
        pkg.GraphCommReLU.from_patterns(1, np.zeros((4, 4), np.int64), np.zeros(4, np.int64))
    with pytest.raises(ValueError, match="needs the labels"):
        pkg.GraphCommReLU.from_patterns(2, np.zeros((4, 4), np.int64))              # a missing y
    with pytest.raises(ValueError, match="has no labels"):
        pkg.GraphCommStep.from_patterns(3, np.zeros((4, 9), np.int64), np.zeros(4, np.int64))     # an extra y
    with pytest.raises(ValueError, match="P = 4 labels"):
        pkg.GraphCommReLU.from_patterns(2, np.zeros((4, 4), np.int64), np.zeros(5, np.int64))
    with pytest.raises(ValueError, match="P x N"):
        pkg.GraphCommStep.from_patterns(1, np.zeros(5, np.int64))                   # a wrong pattern shape
    with pytest.raises(ValueError, match="P x N"):
        pkg.GraphCommStep.from_patterns(1, np.zeros((2, 3, 5), np.int64))
    with pytest.raises(ValueError, match="0/1"):
        pkg.GraphCommStep.from_patterns(1, np.full((2, 3), 2))
    with pytest.raises(ValueError):
        pkg.GraphCommStep(3, 3, 0)
    X = pkg.GraphCommStep(3, 3, 4)
    with pytest.raises(TypeError):
        pkg.GraphCommReLURE(X, 3, 1.0, 1.0)                      # a step graph for the ReLU alias
    with pytest.raises(TypeError):
        pkg.GraphCommStepRE(3, 3, 4, 3, 1.0)                     # neither signature
    with pytest.raises(ValueError, match="greater than 2"):
        pkg.GraphCommStepLE(X, 2, 1.0, 1.0)


def test_ensemble_constructors_share_one_pattern_matrix(pkg):
    X = pkg.GraphCommReLU(4, 2, 9, seed=5)
    for ens, model in ((pkg.GraphCommReLURE, 26), (pkg.GraphCommReLULE, 28)):
        a, b = ens(X, 5, 0.5, 2.0), ens(4, 2, 9, 5, 0.5, 2.0, seed=5)
        assert a.X1 is X and (b.X1.xi == X.xi).all() and (b.X1.y == X.y).all()
        assert a.slice_kind == b.slice_kind == 6 and a.model_kind == b.model_kind == model
        assert a.Nk == 8 and a.M == 5
    fc = pkg.GraphCommStepRE(3, 3, 9, 5, 0.5, 2.0, fc=True, seed=5)
    assert (fc.X1.xi == pkg.GraphCommStep(3, 3, 9, fc=True, seed=5).xi).all()
    S = pkg.GraphCommStep(5, 3, 9)
    for ens, model in ((pkg.GraphCommStepRE, 25), (pkg.GraphCommStepLE, 27)):
        E = ens(S, 3, 0.5, 2.0)
        assert E.slice_kind == 5 and E.model_kind == model and E.Nk == 15
    assert pkg.GraphCommStep.model_kind == 23 and pkg.GraphCommReLU.model_kind == 24
    assert pkg.GraphCommStep.energy_dtype == np.int64 and pkg.GraphCommReLU.energy_dtype == np.int64
