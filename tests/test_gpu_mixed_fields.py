"""GPU parity for GraphAddFields / GraphAddSubFields over a GraphMixed: rrrMC (af_rrr_kernel over the mix) equals the plain-Python
restatement (tests/add_fields_reference.py over tests/mixed_reference.py) bit for bit — spins, sampled energies, accepted and staged counts
and the DeltaECacheCont that ``rrrmc_af_cache`` returns — through both builds that ``rrrmc_af_build`` names, cut and resumed; standardMC on
the wrappers in both of its builds; a hooked run that stops a replica.  The debug checks are on in every run."""
import numpy as np
import pytest

import mixed_instances as MI

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 1, 2


def wrap(pkg, sub, name):
    X = MI.mix(pkg, name)
    return (pkg.GraphAddSubFields if sub else pkg.GraphAddFields)(MI.fields(X.N), X)


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.5], ids=["direct", "default", "staged"])
@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
@pytest.mark.parametrize("name", ["odd15", "even8", "n65"])
def test_rrr_mc_bit_exact(pkg, oracle, name, sub, thr, beta, build):
    iters, step, R = 600, 50, 33 if name == "even8" else 3
    X = wrap(pkg, sub, name)
    out = MI.run_rrr(pkg, X, R, beta, thr, build, [iters], step)
    assert out["Es"].shape == (R, iters // step) and out["Es"].dtype == np.float64
    run = MI.check_rrr(oracle, X, out, R, beta, thr, iters, step)
    if thr == 0.0:
        assert run.staged_its == 0
    if thr == 1.5:
        assert run.staged_its == iters


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
def test_rrr_mc_over_a_cross_entropy_component(pkg, oracle, build):
    X = pkg.GraphAddSubFields(MI.fields(33), MI.mix(pkg, "xentr33"))
    out = MI.run_rrr(pkg, X, 3, 1.0, 0.5, build, [600], 50)
    MI.check_rrr(oracle, X, out, 3, 1.0, 0.5, 600, 50, replicas={0, 2})


@pytest.mark.parametrize("build", [LDS, GLOBAL], ids=["lds", "global"])
def test_cut_and_resumed_runs_equal_the_run_in_one_call(pkg, oracle, build):
    beta, thr, iters, step, R = 1.0, 0.5, 600, 7, 3
    X = wrap(pkg, 1, "odd15")
    whole = MI.run_rrr(pkg, X, R, beta, thr, build, [iters], step)
    cut = MI.run_rrr(pkg, X, R, beta, thr, build, [1, 99, 100, 37, 363], step)
    two = MI.run_rrr(pkg, X, R + 64, beta, thr, build, [iters], step, devices=[0, 0])
    for k in ("Es", "acc", "staged", "Etr"):
        assert (whole[k] == cut[k]).all(), k
        assert (two[k][:R] == whole[k]).all(), k
    assert (whole["C1"].s == cut["C1"].s).all()
    for x, y, z in zip(whole["cache"], cut["cache"], two["cache"]):
        assert (x == y).all() and (z[:R] == x).all()
    MI.check_rrr(oracle, X, whole, R, beta, thr, iters, step, replicas={0, 2})


@pytest.mark.parametrize("build", [MI.THREAD, MI.WAVE], ids=["thread", "wave"])
@pytest.mark.parametrize("sub", [0, 1], ids=["AddFields", "AddSubFields"])
@pytest.mark.parametrize("name", ["odd15", "n65"])
def test_standard_mc_on_the_wrappers(pkg, oracle, name, sub, build):
    X = wrap(pkg, sub, name)
    out = MI.run_standard(pkg, X, 33, 0.7, [399, 7, 594], 7, build=build)          # (cut at sample points: a standardMC call samples every `step` of its own iterations)
    MI.check_standard(oracle, X, out, 33, 0.7, 1000, 7)


@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_a_hooked_run_that_stops_a_replica(pkg, sampler):
    """through the one hooked-run loop: the hook sees the components' energies of the sample, replica 1 stops at its third sample, the
    others are the un-hooked chain"""
    beta, iters, step, R, seed = 1.0, 600, 100, 3, 5
    X = wrap(pkg, 1, "odd15")
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=seed, quiet=True, replicas=R)
    at = {}

    def hook(it, X_, Cfg, acc, E):
        parts = np.atleast_2d(pkg.mixed_energies(X_))
        assert parts.shape == (R, 6)
        tot = parts[:, 0].copy()
        for c in range(1, 6):
            tot = tot + parts[:, c]
        live = np.array([True, it <= 300, True])          # (a stopped replica is shown frozen; the engine's own configuration moves on)
        assert (np.abs(tot - np.asarray(E, np.float64)) < 1e-10)[live].all()          # GraphAddSubFields: the energy is the mix's own
        if it == 300:
            at["s"] = Cfg.s[1].copy()
        return np.array([True, it < 300, True])

    Es1, C1 = run(X, beta, iters, step=step, seed=seed, quiet=True, replicas=R, hook=hook)
    assert len(Es1[0]) == 6 and len(Es1[1]) == 3 and len(Es1[2]) == 6
    assert list(Es1[1]) == list(np.asarray(Es0)[1][:3]) and list(Es1[0]) == list(np.asarray(Es0)[0])
    assert (C1.s[1] == at["s"]).all() and (C1.s[0] == C0.s[0]).all() and (C1.s[2] == C0.s[2]).all()
