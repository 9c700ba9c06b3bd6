"""The `hook` keyword and resumed calls on the ensembles over sparse Float64 slices (GraphEARE, GraphEALE, GraphEATLE on EA(3, 2), M = 3), as
tests/test_gpu_re_hooks.py / test_gpu_le_hooks.py / test_gpu_tle_hooks.py have them for the other slice kinds: a hooked run is the un-hooked
run with the hook called at the reference's sample points, the per-slice energies / cenergy / distances inside the hook are the sample's and
leave the run (the slices' caches included) unchanged, a hook that stops one chain ends it where the restatement does, and a run cut into
resumed calls anywhere is the run made in one call (rrrMC and standardMC)."""
import numpy as np
import pytest

import le_reference as LE
import re_reference as RE
import sparse_slice_reference as SP
import tle_reference as TLE

pytestmark = pytest.mark.gpu

L_, D_, M, GAMMA, LAM, BETA_G = 3, 2, 3, 1.2, 0.4, 1.5
FAMS = ("re", "le", "tle")


def _graphs(pkg, fam):
    X = (pkg.GraphEARE(L_, D_, M, GAMMA, BETA_G, seed=23) if fam == "re" else pkg.GraphEALE(L_, D_, M, GAMMA, BETA_G, seed=23) if fam == "le"
         else pkg.GraphEATLE(L_, D_, M, GAMMA, LAM, BETA_G, seed=23))
    A, J = X.X1.A, X.X1.J
    ref = ((lambda: SP.make_re(A, J, M, GAMMA, BETA_G)) if fam == "re" else (lambda: SP.make_le(A, J, M, GAMMA, BETA_G)) if fam == "le"
           else (lambda: SP.make_tle(A, J, M, GAMMA, LAM, BETA_G)))
    return X, ref


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hooked_run_equals_unhooked_and_observables_in_hook(pkg, fam, sampler):
    beta, iters, step, R = 0.6, 2000, 100, 3
    X, _ = _graphs(pkg, fam)
    A, J, Nk = X.X1.A, X.X1.J, X.Nk
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    seen = []

    def hook(it, X_, Cfg, acc, E):
        for r in range(R):
            s = RE.config_from_chunks(Cfg.s[r], X_.N)
            if fam == "re":
                Es = pkg.REenergies(X_)
                assert Es.shape == (R, M) and Es[r].tolist() == SP.re_energies(A, J, M, s)
            else:
                Es, Ec, D = (pkg.LEenergies if fam == "le" else pkg.TLEenergies)(X_), pkg.cenergy(X_), pkg.distances(X_)
                assert Es.shape == (R, M) and Ec.shape == (R,) and D.shape == (R, M, M)
                assert Es[r].tolist() == SP.le_energies(A, J, M, s)
                assert Ec[r] == SP.cenergy(A, J, M, s)
                assert D[r].tolist() == LE.distances(Nk, M, s)
        seen.append(it)
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all()
    assert (C0.s == C1.s).all()


@pytest.mark.parametrize("fam", FAMS)
def test_stopping_hook_ends_where_the_reference_does(pkg, oracle, fam):
    beta, step = 0.6, 100
    X, ref = _graphs(pkg, fam)
    calls = []
    Es, Cfg = pkg.rrrMC(X, beta, 3000, step=step, seed=19, quiet=True, hook=lambda it, *a: (calls.append(it), it < 700)[1])
    assert calls == list(range(100, 800, 100)) and len(Es[0]) == 7
    N = X.N
    s = RE.config_from_chunks(oracle.init_config(19, 0, N), N)
    Run = {"re": RE.RrrRun, "le": LE.RrrRun, "tle": TLE.RrrRun}[fam]
    run = Run(ref(), s, beta, 19, oracle)
    es = run.run(3000, step, hook=lambda it, s_, acc, E: it < 700)
    assert np.asarray(Es[0]).tolist() == [float(e) for e in es]
    assert (Cfg.s[0] == RE.chunks_from_config(s)).all()


@pytest.mark.parametrize("fam", FAMS)
def test_run_cut_into_resumed_calls_equals_one_call(pkg, fam):
    R, beta, step, total = 4, 0.6, 50, 2000
    X, _ = _graphs(pkg, fam)
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
                pa, pb = (a.tle_cache(), b.tle_cache()) if fam == "tle" else (a.rrr_cache(), b.rrr_cache())
                assert (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
