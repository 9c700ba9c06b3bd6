"""CPU checks of the Topological Local Entropy ensemble (src/graphs/TLE.jl): the plain-Python restatement (tests/tle_reference.py) against
the definitions — both integer caches after random move sequences with immediate undos, delta_energy against energy differences,
hand-enumerated energies — and the library's host-only entry points (rrrmc_tle_tables, rrrmc_tle_check_topology) and Python aliases
against the restatement.  No GPU."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

import tle_reference as TLE
from le_reference import findk


def _ring(Nk):
    return [[(i - 1) % Nk, (i + 1) % Nk] for i in range(Nk)]


def _csr(neighb):
    rowptr = np.zeros(len(neighb) + 1, np.int32)
    rowptr[1:] = np.cumsum([len(n) for n in neighb])
    cols = np.array([j for n in neighb for j in n] or [0], np.int32)
    return rowptr, cols


@pytest.mark.parametrize("Nk,M,neighb", [(5, 3, "ring"), (6, 4, "all"), (7, 5, "ragged"), (4, 3, "empty")])
def test_incremental_caches_equal_the_definition_and_delta_is_the_energy_difference(Nk, M, neighb):
    rnd = random.Random(1000 * Nk + M)
    nb = {"ring": _ring(Nk), "all": [[j for j in range(Nk) if j != i] for i in range(Nk)], "empty": [[] for _ in range(Nk)],
          "ragged": [[1, 2, 3], [0], [0, 3], [2, 0], [], [6], [5]]}[neighb]
    gT, lT = 0.75, -0.3
    X = TLE.GraphTLE(Nk, M, gT, lT, nb)
    s = np.array([rnd.randrange(2) for _ in range(X.N)], np.int64)
    X.energy(s)
    assert (X.lf1, X.lf2) == X.fields_of(s)
    last = None
    for step in range(400):
        move = last if (last is not None and rnd.random() < 0.3) else rnd.randrange(X.N)      # immediate undos take the swap path
        d = X.delta(move)
        Y = TLE.GraphTLE(Nk, M, gT, lT, nb)
        E0 = Y.energy(s)
        s[move] ^= 1
        X.update_cache(s, move)
        E1 = Y.energy(s)
        assert (X.lf1, X.lf2) == X.fields_of(s), (step, move)
        assert (Y.lf1, Y.lf2) == (X.lf1, X.lf2)
        assert abs(d - (E1 - E0)) < 1e-12 * max(1.0, abs(E0), abs(E1)), (step, move)
        last = move
    # the centre's topological field is the sum of its replicas'
    for i in range(Nk):
        assert X.lf2[i * (M + 1)] == sum(X.lf2[i * (M + 1) + k] for k in range(1, M + 1))


def test_hand_enumerated_energies_nk2_m3():
    # Nk = 2, M = 3, ∂0 = {1}, ∂1 = {0}: E0 = -γT Σ_i σc_i μ_i - λT σc_0 σc_1 Σ_k σ_(0,k) σ_(1,k)
    gamma, lam, beta = 0.6, 0.4, 1.2
    gT, lT = gamma / beta, lam / beta
    for bits in itertools.product((0, 1), repeat=8):
        s = np.array(bits, np.int64)
        sg = 2 * s - 1
        n = -(sg[0] * (sg[1] + sg[2] + sg[3]) + sg[4] * (sg[5] + sg[6] + sg[7]))
        r = -sg[0] * sg[4] * (sg[1] * sg[5] + sg[2] * sg[6] + sg[3] * sg[7])
        X = TLE.TopologicalLocalEntropy(2, 3, gamma, lam, beta, "empty", neighb=[[1], [0]])
        assert X.energy(s.copy()) == int(n) * gT + int(r) * lT
        for j in range(8):
            t = s.copy()
            t[j] ^= 1
            sgt = 2 * t - 1
            nt = -(sgt[0] * (sgt[1] + sgt[2] + sgt[3]) + sgt[4] * (sgt[5] + sgt[6] + sgt[7]))
            rt = -sgt[0] * sgt[4] * (sgt[1] * sgt[5] + sgt[2] * sgt[6] + sgt[3] * sgt[7])
            assert abs(X.delta(j) - ((int(nt) - int(n)) * gT + (int(rt) - int(r)) * lT)) < 1e-14


def test_neighbors_order():
    X = TLE.GraphTLE(4, 3, 1.0, 1.0, [[2, 1], [0], [0], []])
    assert X.neighbors(0) == [1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7]          # replicas, then the intervals of 2 and 1, centre first
    assert X.neighbors(2) == [0, 8, 10, 4, 6]                             # the centre, then (centre of i1, (i1, k)) in list order
    assert X.neighbors(12) == [13, 14, 15] and X.neighbors(13) == [12]


TABLE_CASES = [(3, 0.9, 0.3, 1.2, 2), (4, 1.5, 0.5, 2.0, 9), (8, 1.5, 0.5, 2.0, 9), (5, 0.7, 0.7, 1.0, 4), (6, 1.1, 0.0, 0.9, 3),
               (7, 0.0, 0.8, 1.3, 5), (3, -0.6, 0.4, 1.2, 1), (4, 0.6, -0.4, -1.2, 6), (9, 0.31, 0.17, 0.77, 12), (5, 1.0, 0.25, 1.0, 60),
               (3, 1.0, 0.5, 1.0, 0), (31, 0.2, 0.1, 1.0, 3), (3, 0.0, 0.0, 1.0, 2)]


@pytest.mark.parametrize("M,gamma,lam,beta,maxdeg", TABLE_CASES)
def test_tle_tables_equal_all_delta_e_and_every_field_pair_has_a_level(pkg, M, gamma, lam, beta, maxdeg):
    L = C.c_int64(-1)
    assert pkg.lib().rrrmc_tle_tables(M, gamma, lam, beta, maxdeg, None, C.byref(L)) == 0
    ref = TLE.all_delta_e(M, gamma / beta, lam / beta, maxdeg)
    assert L.value == len(ref)
    dE = np.full(L.value + 1, np.nan)
    assert pkg.lib().rrrmc_tle_tables(M, gamma, lam, beta, maxdeg, dE.ctypes.data, C.byref(L)) == 0
    assert dE[:L.value].tolist() == ref and np.isnan(dE[L.value])
    # every field pair the ensemble can take: a replica's (±1, |lf2| <= deg), a centre's (parity of M, |lf2| <= M deg)
    gT, lT = gamma / beta, lam / beta
    pairs = [(a, b) for a in (-1, 1) for b in range(-maxdeg, maxdeg + 1)]
    pairs += [(a, b) for a in range(-M, M + 1, 2) for b in range(-M * maxdeg, M * maxdeg + 1)]
    for a, b in pairs:
        d = (2 * gT) * a + (2 * lT) * b
        k = findk(ref, d)
        assert k > 0 and ref[k - 1] == abs(d), (a, b)


def test_tle_tables_known_sizes_and_refusals(pkg):
    L = C.c_int64(0)
    assert pkg.lib().rrrmc_tle_tables(3, 0.75, 0.25, 1.0, 9, None, C.byref(L)) == 0 and L.value == 37      # SK slices, Nk = 10, M = 3
    assert pkg.lib().rrrmc_tle_tables(2, 1.0, 1.0, 1.0, 3, None, C.byref(L)) == 1          # M > 2 (TLE.jl:29)
    assert pkg.lib().rrrmc_tle_tables(32, 1.0, 1.0, 1.0, 3, None, C.byref(L)) == 3         # beyond the kernels
    assert pkg.lib().rrrmc_tle_tables(3, 1.0, 1.0, 0.0, 3, None, C.byref(L)) == 1          # γ / β not finite


def _check(pkg, neighb, Nk=None):
    rowptr, cols = _csr(neighb)
    md = C.c_int64(-1)
    rc = pkg.lib().rrrmc_tle_check_topology(len(neighb) if Nk is None else Nk, rowptr, cols, C.byref(md))
    return rc, md.value, pkg.lib().rrrmc_last_error(None).decode()


def test_check_topology_accepts_and_refuses_as_the_reference(pkg):
    assert _check(pkg, _ring(5))[:2] == (0, 2)
    assert _check(pkg, [[], [], []])[:2] == (0, 0)
    bad = {"asym": [[1], [], [0]], "self": [[0, 1], [0]], "dup": [[1, 2, 1], [0], [0]], "range": [[3], [0], []], "neg": [[-1], [], []]}
    for name, nb in bad.items():
        rc, _, msg = _check(pkg, nb)
        assert rc == 1, name
        with pytest.raises(ValueError) as e:
            TLE.check_neighb(len(nb), 3, nb)
        assert msg == str(e.value), name                       # the reference's wording, 1-based
    assert "not symmetrical, 2 ∈ ∂1 but 1 ∉ ∂2" in _check(pkg, bad["asym"])[2]
    assert "duplicated element 1 in neighb[1]" in _check(pkg, bad["dup"])[2]
    # a duplicate pair met later in the first index but earlier in the scan: the reference names the smaller first index
    assert "duplicated element 1 in neighb[1]" in _check(pkg, [[1, 2, 2, 1], [0], [0]])[2]


def test_python_constructor_checks(pkg):
    with pytest.raises(ValueError, match="M must be greater than 2"):
        pkg.Graph0TLE(4, 2, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="expected 5 spins, got 4"):
        pkg.GraphTopologicalLocalEntropy(5, 3, 1.0, 1.0, 1.0, pkg.GraphSK(4, seed=1))
    with pytest.raises(TypeError):
        pkg.GraphTopologicalLocalEntropy(5, 3, 1.0, 1.0, 1.0, pkg.GraphPercStep(5, 3, seed=1))
    with pytest.raises(ValueError, match="expected length"):
        TLE.check_neighb(3, 3, [[], []])


def test_python_aliases(pkg):
    X0 = pkg.Graph0TLE(4, 5, 2.0, 0.5, 0.4)
    assert (X0.N, X0.Nk, X0.model_kind, X0.max_deg) == (24, 4, 44, 0) and X0.neighb == [[], [], [], []]
    assert X0.gammaT == 2.0 / 0.4 and X0.lambdaT == 0.5 / 0.4
    Xs = pkg.GraphSKTLE(6, 3, 1.0, 0.5, 1.0, seed=2)
    assert Xs.model_kind == 45 and Xs.N == 24 and Xs.neighb == [[j for j in range(6) if j != i] for i in range(6)]
    assert (Xs.J == pkg.GraphSK(6, seed=2).J).all()
    assert pkg.GraphTopologicalLocalEntropy(6, 3, 1.0, 0.5, 1.0, pkg.GraphSKNormal(6, seed=2)).model_kind == 46
    S = pkg.GraphSAT.from_clauses(5, [[0, 1], [1, 2, 3], [3]], [[1, 0], [0, 0, 1], [1]])
    Xt = pkg.GraphSATTLE(S, 3, 0.6, 0.4, 1.2)
    assert Xt.model_kind == 47 and Xt.X1 is S and Xt.Nk == 5 and Xt.N == 20
    assert Xt.neighb == [[1], [0, 2, 3], [1, 3], [1, 2], []] == S.neighb
    Xr = pkg.GraphSATTLE(20, 3, 4.2, 3, 0.6, 0.4, 1.2, seed=7)
    assert Xr.Nk == 20 and Xr.X1.M == 84 and Xr.neighb == pkg.GraphSAT(20, 3, 4.2, seed=7).neighb
    assert Xs.tables().tolist() == TLE.all_delta_e(3, 1.0, 0.5, 5)
    for f in (pkg.TLEenergies, pkg.cenergy, pkg.distances):
        with pytest.raises(RuntimeError):
            f(X0)
    for name in ("GraphTopologicalLocalEntropy", "Graph0TLE", "GraphSKTLE", "GraphSATTLE", "TLEenergies"):
        assert name in pkg.__all__
