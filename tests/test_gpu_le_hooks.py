"""Hooks, resumed calls and the stationary distribution on the Local Entropy ensemble (DESIGN §4j applied to src/graphs/LE.jl): a hooked run
is the un-hooked run, a run cut into resumed calls anywhere is the run made in one call, a stopping hook ends the chain where the reference
does, LEenergies / cenergy / distances inside the hook are the sample's, a two-shard context equals the single one, the debug checks stay
clean — and the final configurations of many independent chains follow exp(−β E) / Z exactly (χ², independent of the restatement)."""
import itertools

import numpy as np
import pytest

import le_reference as LE

pytestmark = pytest.mark.gpu


def _skn(pkg, Nk, M):
    return pkg.GraphLocalEntropy(Nk, M, 1.5, 2.0, pkg.GraphSKNormal(Nk, seed=17))


@pytest.mark.parametrize("kind", ["sk", "skn"])
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hooked_run_equals_unhooked_and_observables_in_hook(pkg, kind, sampler):
    Nk, M, beta, iters, step, R = 12, 5, 1.3, 4000, 100, 3
    X = pkg.GraphSKLE(Nk, M, 1.5, 2.0, seed=23) if kind == "sk" else _skn(pkg, Nk, M)
    J = X.J
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    seen = []

    def hook(it, X_, Cfg, acc, E):
        LEs, Ec, D = pkg.LEenergies(X_), pkg.cenergy(X_), pkg.distances(X_)
        assert LEs.shape == (R, M) and Ec.shape == (R,) and D.shape == (R, M, M)
        for r in range(R):
            s = LE.config_from_chunks(Cfg.s[r], X_.N)
            assert LEs[r].tolist() == LE.le_energies(Nk, M, kind, J, s)
            assert Ec[r] == LE.cenergy(Nk, M, kind, J, s)
            assert D[r].tolist() == LE.distances(Nk, M, s)
        seen.append(it)
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all()
    assert (C0.s == C1.s).all()


def test_observables_single_replica_shapes(pkg):
    X = pkg.GraphSKLE(16, 4, 1.0, 1.0, seed=5)
    shapes = []
    pkg.rrrMC(X, 1.0, 300, step=100, seed=3, quiet=True,
              hook=lambda it, X_, C_, a, E: shapes.append((pkg.LEenergies(X_).shape, type(pkg.cenergy(X_)), pkg.distances(X_).shape)) or True)
    assert shapes == [((4,), float, (4, 4))] * 3


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, kind):
    Nk, M, R, beta, step, total = 9, 6, 4, 1.1, 50, 3000
    X = pkg.Graph0LE(Nk, M, 1.5, 2.0) if kind == "empty" else pkg.GraphSKLE(Nk, M, 1.5, 2.0, seed=4) if kind == "sk" else _skn(pkg, Nk, M)
    rng = np.random.default_rng(12)
    cuts = sorted(set(rng.integers(1, total, 7).tolist()))
    pieces = np.diff([0] + cuts + [total]).tolist()
    with pkg.Engine(X, R) as a, pkg.Engine(X, R) as b:
        for e in (a, b):
            e.seed(31)
            e.init_spins_random()
        Ea, acca, sta = a.rrr_mc(beta, total, step)
        b.set_resume(True)
        Es, acc, st = [], np.zeros(R, np.int64), np.zeros(R, np.int64)
        for n in pieces:
            e_, ac, s_ = b.rrr_mc(beta, n, step)
            Es.append(e_)
            acc += ac
            st += s_
        Eb = np.concatenate(Es, axis=1)
        assert (Ea == Eb).all() and (acca == acc).all() and (sta == st).all()
        assert (a.get_config().s == b.get_config().s).all()
        pa, pb = a.rrr_cache(), b.rrr_cache()
        assert (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
        assert (a.run_energy() == b.run_energy()).all()


def test_stopping_hook_ends_where_the_reference_does(pkg, oracle):
    Nk, M, beta, step = 10, 8, 2.0, 100
    X = pkg.GraphSKLE(Nk, M, 1.5, 2.0, seed=8)
    calls = []
    Es, Cfg = pkg.rrrMC(X, beta, 5000, step=step, seed=19, quiet=True, hook=lambda it, *a: (calls.append(it), it < 700)[1])
    assert calls == list(range(100, 800, 100)) and len(Es[0]) == 7
    # the restatement stops at the same sample: the configuration is the one the hook saw at it = 700
    N = Nk * (M + 1)
    X2 = LE.make_ensemble(Nk, M, 1.5, 2.0, "sk", X.J)
    s = LE.config_from_chunks(oracle.init_config(19, 0, N), N)
    run = LE.RrrRun(X2, s, beta, 19, oracle)
    es = run.run(5000, step, hook=lambda it, s_, acc, E: it < 700)
    assert np.asarray(Es[0]).tolist() == es
    assert (Cfg.s[0] == LE.chunks_from_config(s)).all()


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_two_shard_context_equals_single(pkg, kind):
    X = pkg.Graph0LE(20, 5, 2.0, 0.4) if kind == "empty" else pkg.GraphSKLE(20, 5, 2.0, 0.4, seed=2) if kind == "sk" else _skn(pkg, 12, 4)
    res = []
    for devices in (None, [0, 0]):
        with pkg.Engine(X, 70, devices=devices) as eng:
            eng.seed(5)
            eng.init_spins_random()
            r1 = eng.rrr_mc(0.4, 3000, 100)
            cache = eng.rrr_cache()
            r2 = eng.standard_mc(0.4, 3000, 100)
            res.append((r1, r2, cache, eng.get_config().s.copy(), eng.le_energies(), eng.cenergy(), eng.distances()))
    (a1, a2, pa, *oa), (b1, b2, pb, *ob) = res
    for x, y in zip(a1 + a2 + pa + tuple(oa), b1 + b2 + pb + tuple(ob)):
        assert (np.asarray(x) == np.asarray(y)).all()


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_debug_checks_pass_on_a_run(pkg, kind):
    X = pkg.Graph0LE(8, 4, 1.5, 2.0) if kind == "empty" else pkg.GraphSKLE(8, 5, 1.5, 2.0, seed=1) if kind == "sk" else _skn(pkg, 8, 4)
    with pkg.Engine(X, 3) as eng:
        eng.set_debug_checks(True)
        eng.seed(2)
        eng.init_spins_random()
        eng.rrr_mc(1.0, 2000, 100, staged_thr=0.5)
        eng.rrr_mc(1.0, 2000, 100, staged_thr=1.0)
        eng.standard_mc(1.0, 2000, 100)
        tot, sw, nl = eng.last_timing()
        assert nl == 1 and sw > 0
        eng.get_config()                     # a mismatch would surface here as an RRRMCError


# ---- the stationary distribution ---------------------------------------------------------------------------------------------------
def _energy_from_definition(Nk, M, gT, J, s):
    """E = -γT Σ_i σc μ_i + Σ_k E_k (GraphSKNormal slices: -Σ_{a<b} J_ab σa σb), the centre's own energy left out"""
    R = M + 1
    sg = 2 * np.asarray(s) - 1
    E = 0.0
    for i in range(Nk):
        E -= gT * sg[i * R] * sum(sg[i * R + k] for k in range(1, R))
    for k in range(1, R):
        E += -sum(J[a][b] * sg[a * R + k] * sg[b * R + k] for a in range(Nk) for b in range(a + 1, Nk))
    return E


@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_final_configurations_follow_the_boltzmann_distribution(pkg, oracle, sampler):
    # GraphLocalEntropy(2, 3, γ, β, GraphSKNormal): N = 8, 256 states; 65 536 independent chains, one final configuration each
    Nk, M, gamma, beta_g, beta, R = 2, 3, 0.6, 1.2, 0.6, 65536
    J = oracle.gen_sk_gauss(Nk, 21)
    X = pkg.GraphLocalEntropy(Nk, M, gamma, beta_g, pkg.GraphSKNormal.from_J(J))
    N = X.N
    states = list(itertools.product((0, 1), repeat=N))
    E = np.array([_energy_from_definition(Nk, M, gamma / beta_g, J, s) for s in states])
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    expected = p * R
    assert expected.min() >= 5                         # every bin is a valid χ² term
    with pkg.Engine(X, R) as eng:
        eng.seed(424242)
        eng.init_spins_random()
        if sampler == "rrr":
            eng.rrr_mc(beta, 4000, 4000)
        else:
            eng.standard_mc(beta, 4000, 4000)
        Cfg = eng.get_config()
        # the tracked energies are the energies of the final configurations
        idx = np.zeros(R, np.int64)
        for j in range(N):                             # state index: site 0 is the most significant bit, as itertools.product orders them
            idx = idx * 2 + ((Cfg.s[:, 0] >> np.uint64(j)) & np.uint64(1)).astype(np.int64)
        assert np.abs(eng.run_energy() - E[idx]).max() < 1e-12
    counts = np.bincount(idx, minlength=len(states))
    stat = float(((counts - expected) ** 2 / expected).sum())
    # the χ² quantile of the 1e-6 upper tail, Wilson-Hilferty (z = 4.7534 is the normal 1e-6 quantile; for 255 degrees of freedom: 377.2)
    k = len(states) - 1
    limit = k * (1 - 2 / (9 * k) + 4.753424 * (2 / (9 * k)) ** 0.5) ** 3
    assert stat < limit, (stat, limit)
