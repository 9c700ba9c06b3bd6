"""CPU checks of the Local Entropy ensemble (src/graphs/LE.jl): the library's host-only table (rrrmc_le_tables) against allΔE restated from
LE.jl:176-179, and the plain-Python restatement (tests/le_reference.py) against what the reference pins — tracked E == energy(X, C)
(RRRMC.jl:250), check_consistency (DeltaE.jl:120-135), hand-enumerated energies, GraphLE's fields as a function of the spins.  No GPU."""
import itertools
import math
import random

import numpy as np
import pytest

import le_reference as LE


@pytest.mark.parametrize("gamma,beta", [(2.0, 0.4), (1.5, 2.0), (-0.7, 1.3), (0.3, -1.0), (0.0, 1.0), (-0.0, 2.0)])
def test_le_tables_equal_all_delta_e(pkg, gamma, beta):
    for M in range(3, 13):
        L = M // 2 + 2 if M % 2 == 0 else (M + 1) // 2
        dE = np.full(M // 2 + 2, np.nan)
        assert pkg.lib().rrrmc_le_tables(M, gamma, beta, dE) == 0
        ref = LE.all_delta_e(M, gamma / beta)
        assert len(ref) == L
        assert dE[:L].tolist() == ref, (M, gamma, beta)
        assert np.isnan(dE[L:]).all()                # nothing written beyond L
    X = pkg.Graph0LE(4, 6, gamma, beta)
    assert X.tables().tolist() == LE.all_delta_e(6, gamma / beta)


def test_le_tables_refuse_M_bounds(pkg):
    dE = np.zeros(32, np.float64)
    assert pkg.lib().rrrmc_le_tables(2, 1.0, 1.0, dE) == 1          # M > 2 (LE.jl:24)
    assert pkg.lib().rrrmc_le_tables(32, 1.0, 1.0, dE) == 3         # beyond the kernels
    assert pkg.lib().rrrmc_le_tables(31, 1.0, 1.0, dE) == 0


def test_findk_with_repeated_zeros_follows_the_probe_order():
    # γ = 0: every allΔE entry is 0 and findk returns the first index its generated search compares equal
    for M in range(3, 32):
        ae = LE.all_delta_e(M, 0.0)
        L = len(ae)
        k = LE.findk(ae, 0.0)
        assert k == (1 if L <= 10 else (1 + L) // 2), (M, k)
    # γ ≠ 0: the level of every field value the ensemble can take
    for M in range(3, 32):
        gT = 1.7
        ae = LE.all_delta_e(M, gT)
        for lf in range(-M, M + 1):
            if lf in (1, -1) or (lf - M) % 2 == 0:
                assert ae[LE.findk(ae, 2 * gT * lf) - 1] == abs(2 * gT * lf)


def test_graph_objects(pkg):
    X = pkg.Graph0LE(4, 5, 2.0, 0.4)
    assert X.N == 24 and X.model_kind == 14 and X.gammaT == 2.0 / 0.4
    assert pkg.GraphSKLE(8, 3, 1.0, 1.0, seed=2).model_kind == 15
    assert pkg.GraphLocalEntropy(8, 3, 1.0, 1.0, pkg.GraphSKNormal(8, seed=2)).model_kind == 16
    with pytest.raises(ValueError):
        pkg.Graph0LE(4, 2, 2.0, 0.4)
    for f in (pkg.LEenergies, pkg.cenergy, pkg.distances):
        with pytest.raises(RuntimeError):
            f(X)                             # no engine runs it, no configuration given: no stale data


def test_graph0le_small_known_energies():
    # Graph0LE(1, 3): one centre spin and three replicas; E = -γT σc (σ1 + σ2 + σ3) over all 16 configurations
    gamma, beta = 1.5, 2.0
    gT = gamma / beta
    for bits in itertools.product((0, 1), repeat=4):
        s = np.array(bits, np.int64)
        sg = 2 * s - 1
        X = LE.make_ensemble(1, 3, gamma, beta, "empty")
        assert X.energy(s.copy()) == -gT * sg[0] * (sg[1] + sg[2] + sg[3])
        for j in range(4):
            t = s.copy()
            t[j] ^= 1
            assert X.delta(j) == LE.energy_fresh(1, 3, gamma, beta, "empty", None, t) - X.energy(s.copy())


def _brute_energy(Nk, M, gamma, beta, kind, J, s):
    """energy(X, C) from the definitions: -γT Σ_i σc μ_i + Σ_k E_slice(k); the centre's own energy left out"""
    gT = gamma / beta
    R = M + 1
    E = 0.0
    for i in range(Nk):
        sc = 2 * int(s[i * R]) - 1
        E -= gT * sc * sum(2 * int(s[i * R + k]) - 1 for k in range(1, R))
    for k in range(1, R):
        sl = [2 * int(s[i * R + k]) - 1 for i in range(Nk)]
        if kind == "skn":
            E += -sum(J[a][b] * sl[a] * sl[b] for a in range(Nk) for b in range(a + 1, Nk))
        elif kind == "sk":
            Jb = [[(int(J[a, b >> 6]) >> (b & 63)) & 1 for b in range(Nk)] for a in range(Nk)]
            E += -sum((2 * Jb[a][b] - 1) * sl[a] * sl[b] for a in range(Nk) for b in range(a + 1, Nk)) / math.sqrt(Nk)
    return E


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_hand_enumerated_energies_nk2_m3(oracle, kind):
    Nk, M, gamma, beta = 2, 3, 1.5, 2.0
    J = None if kind == "empty" else oracle.gen_sk_binary(Nk, 11) if kind == "sk" else oracle.gen_sk_gauss(Nk, 11)
    for bits in itertools.product((0, 1), repeat=Nk * (M + 1)):
        s = np.array(bits, np.int64)
        X = LE.make_ensemble(Nk, M, gamma, beta, kind, J)
        E = X.energy(s.copy())
        assert abs(E - _brute_energy(Nk, M, gamma, beta, kind, J, s)) < 1e-12
        for j in range(Nk * (M + 1)):        # delta_energy(X, C, j) = energy after the flip − energy before (LE.jl:292-295)
            t = s.copy()
            t[j] ^= 1
            assert abs(X.delta(j) - (_brute_energy(Nk, M, gamma, beta, kind, J, t) - E)) < 1e-12


@pytest.mark.parametrize("M", [3, 4, 7, 8])
def test_lfields_equal_the_spin_function_after_flips_and_undos(M):
    # update_cache! (LE.jl:92-154) with its move_last swap keeps lfields = σc σ_(i,k) / σc μ_i: random flips, immediate undos, repeated
    # flips of one site and runs of the same move, as rrrMC's compute_staged! and apply_move! produce them
    rng = random.Random(M)
    Nk = 5
    G = LE.GraphLE(Nk, M, 0.75)
    s = np.array([rng.randint(0, 1) for _ in range(G.N)], np.int64)
    G.energy(s)
    assert G.lfields == G.fields_of(s)
    last = 0
    for step in range(4000):
        r = rng.random()
        move = last if r < 0.4 else rng.randrange(G.N)
        reps = 1 if r < 0.8 else rng.randint(2, 4)
        for _ in range(reps):
            s[move] ^= 1
            G.update_cache(s, move)
            assert G.lfields == G.fields_of(s), (step, move)
        last = move


@pytest.mark.parametrize("kind,Nk,M,thr", [("empty", 6, 5, 0.5), ("sk", 10, 8, 0.5), ("skn", 7, 4, 1.0), ("sk", 9, 7, 0.0),
                                           ("skn", 5, 3, 0.5), ("skn", 4, 6, 0.0)])
def test_restatement_tracks_energy_and_stays_consistent(oracle, kind, Nk, M, thr):
    seed = 1877 + Nk * M
    gamma, beta_g, beta = 1.5, 2.0, 1.3
    J = None if kind == "empty" else oracle.gen_sk_binary(Nk, seed) if kind == "sk" else oracle.gen_sk_gauss(Nk, seed)
    N = Nk * (M + 1)
    X = LE.make_ensemble(Nk, M, gamma, beta_g, kind, J)
    s = LE.config_from_chunks(oracle.init_config(seed, 0, N), N)
    run = LE.RrrRun(X, s, beta, seed, oracle, staged_thr=thr)
    for _ in range(600):                     # the tracked E against a fresh energy(X, C) after every iteration (RRRMC.jl:250)
        run.run(1, 50)
        assert abs(run.E - LE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s)) < 1e-10
        assert X.X0.lfields == X.X0.fields_of(s)
    assert run.accepted > 0
    run.cache.check(s)
    run.run(3000, 100)
    run.cache.check(s)
    assert X.X0.lfields == X.X0.fields_of(s)
    assert abs(run.E - LE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s)) < 1e-10
    # standardMC: tracked E after every piece
    X2 = LE.make_ensemble(Nk, M, gamma, beta_g, kind, J)
    s2 = LE.config_from_chunks(oracle.init_config(seed, 1, N), N)
    E = None
    for part in range(6):
        _, E, acc = LE.standard_mc(X2, s2, beta, 200, 10, seed, oracle, replica=1, it0=200 * part, E=E)
        assert abs(E - LE.energy_fresh(Nk, M, gamma, beta_g, kind, J, s2)) < 1e-10


def test_restatement_with_gamma_zero(oracle):
    # γ = 0: all levels coincide; the restatement still classifies by findk's probe order and tracks E
    Nk, M = 6, 4
    J = oracle.gen_sk_gauss(Nk, 5)
    X = LE.make_ensemble(Nk, M, 0.0, 1.0, "skn", J)
    N = Nk * (M + 1)
    s = LE.config_from_chunks(oracle.init_config(5, 0, N), N)
    run = LE.RrrRun(X, s, 1.1, 5, oracle)
    run.run(2000, 100)
    run.cache.check(s)
    assert abs(run.E - LE.energy_fresh(Nk, M, 0.0, 1.0, "skn", J, s)) < 1e-10


def test_observables_restated():
    s = np.array([1, 0, 1, 1, 0, 1, 1, 0], np.int64)          # Nk = 2, M = 3: centre (1, 0), replicas (0,1) (1,1) (1,0)
    assert LE.distances(2, 3, s) == [[0, 1, 2], [1, 0, 1], [2, 1, 0]]
    assert LE.le_energies(2, 3, "empty", None, s) == [0.0, 0.0, 0.0] and LE.cenergy(2, 3, "empty", None, s) == 0.0
