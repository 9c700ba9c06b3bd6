"""The `hook` keyword on the Topological Local Entropy ensemble, as tests/test_gpu_le_hooks.py has it for GraphLocalEntropy: a hooked run is
the un-hooked run, TLEenergies / cenergy / distances inside the hook are the sample's and leave the run unchanged, a stopping hook ends the
chain where the restatement does, and a run cut into resumed calls anywhere is the run made in one call (rrrMC and standardMC)."""
import numpy as np
import pytest

import sat_reference as SR
import tle_reference as TLE

pytestmark = pytest.mark.gpu


def _graphs(pkg, kind, Nk, M):
    if kind == "sk":
        X = pkg.GraphSKTLE(Nk, M, 1.5, 0.5, 2.0, seed=23)
        return X, lambda: TLE.TopologicalLocalEntropy(Nk, M, 1.5, 0.5, 2.0, "sk", X.J)
    if kind == "skn":
        X = pkg.GraphTopologicalLocalEntropy(Nk, M, 1.5, 0.5, 2.0, pkg.GraphSKNormal(Nk, seed=17))
        return X, lambda: TLE.TopologicalLocalEntropy(Nk, M, 1.5, 0.5, 2.0, "skn", X.J)
    sat = SR.ragged_instance()
    X = pkg.GraphSATTLE(pkg.GraphSAT.from_clauses(*sat), M, 1.5, 0.5, 2.0)
    return X, lambda: TLE.TopologicalLocalEntropy(sat[0], M, 1.5, 0.5, 2.0, "sat", None, sat)


@pytest.mark.parametrize("kind", ["sk", "skn", "sat"])
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hooked_run_equals_unhooked_and_observables_in_hook(pkg, kind, sampler):
    Nk, M, beta, iters, step, R = (20 if kind == "sat" else 12), 4, 1.3, 2000, 100, 3
    X, ref = _graphs(pkg, kind, Nk, M)
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    seen = []
    Xr = ref()

    def hook(it, X_, Cfg, acc, E):
        Es, Ec, D = pkg.TLEenergies(X_), pkg.cenergy(X_), pkg.distances(X_)
        assert Es.shape == (R, M) and Ec.shape == (R,) and D.shape == (R, M, M)
        for r in range(R):
            s = TLE.config_from_chunks(Cfg.s[r], X_.N)
            assert Es[r].tolist() == TLE.tle_energies(Xr, s)
            assert Ec[r] == TLE.cenergy(Xr, s)
            assert D[r].tolist() == TLE.distances(Nk, M, s)
        seen.append(it)
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all()
    assert (C0.s == C1.s).all()


def test_stopping_hook_ends_where_the_reference_does(pkg, oracle):
    Nk, M, beta, step = 10, 8, 2.0, 100
    X, ref = _graphs(pkg, "sk", Nk, M)
    calls = []
    Es, Cfg = pkg.rrrMC(X, beta, 3000, step=step, seed=19, quiet=True, hook=lambda it, *a: (calls.append(it), it < 700)[1])
    assert calls == list(range(100, 800, 100)) and len(Es[0]) == 7
    N = Nk * (M + 1)
    s = TLE.config_from_chunks(oracle.init_config(19, 0, N), N)
    run = TLE.RrrRun(ref(), s, beta, 19, oracle)
    es = run.run(3000, step, hook=lambda it, s_, acc, E: it < 700)
    assert np.asarray(Es[0]).tolist() == es
    assert (Cfg.s[0] == TLE.chunks_from_config(s)).all()


@pytest.mark.parametrize("kind", ["sk", "skn", "sat"])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, kind):
    M, R, beta, step, total = 5, 4, 1.1, 50, 2000
    X, _ = _graphs(pkg, kind, 20 if kind == "sat" else 9, M)
    rng = np.random.default_rng(12)
    cuts = sorted(set(rng.integers(1, total, 7).tolist()))
    pieces = np.diff([0] + cuts + [total]).tolist()
    for sampler in ("rrr", "std"):
        with pkg.Engine(X, R) as a, pkg.Engine(X, R) as b:
            for e in (a, b):
                e.seed(31)
                e.init_spins_random()
            call = (lambda e, n: e.rrr_mc(beta, n, step)) if sampler == "rrr" else (lambda e, n: e.standard_mc(beta, n, step) + (np.zeros(R, np.int64),))
            Ea, acca, sta = call(a, total)
            b.set_resume(True)
            Es, acc, st = [], np.zeros(R, np.int64), np.zeros(R, np.int64)
            for n in pieces:
                e_, ac, s_ = call(b, n)
                Es.append(e_)
                acc += ac
                st += s_
            Eb = np.concatenate(Es, axis=1)
            if sampler == "rrr":                     # (standardMC samples by the call's own iteration count: the pieces' samples differ)
                assert (Ea == Eb).all()
            assert (acca == acc).all() and (sta == st).all()
            assert (a.get_config().s == b.get_config().s).all()
            assert (a.run_energy() == b.run_energy()).all()
            if sampler == "rrr":
                pa, pb = a.tle_cache(), b.tle_cache()
                assert (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
