"""Hooks on GraphAddFields / GraphAddSubFields through the front end's hooked-run loop: ``hook(it, X, C, acc, E)`` is called at the
reference's sample points (src/RRRMC.jl:253-256, :104-108), a hooked run is the un-hooked chain bit for bit, what the hook sees is the
restatement's state at that sample, and a replica stops when its hook returns False."""
import numpy as np
import pytest

import add_fields_reference as AF
import re_reference as RE
from test_gpu_add_fields_parity import wrap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sampler", ["rrr", "std"])
@pytest.mark.parametrize("name,sub", [("sat33", 1), ("perc", 0)])
def test_hooked_run_equals_unhooked_and_sees_the_samples(pkg, oracle, name, sub, sampler):
    beta, iters, step, R, seed = 1.0, 700, 100, 3, 77
    X = wrap(pkg, sub, name)
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=seed, quiet=True, replicas=R)
    seen = []

    def hook(it, X_, Cfg, acc, E):
        assert X_ is X
        seen.append((it, Cfg.s.copy(), np.array(acc), np.array(E)))
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=seed, quiet=True, replicas=R, hook=hook)
    assert [h[0] for h in seen] == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all() and (C0.s == C1.s).all()
    # the restatement from the same start: replica 0's hook arguments
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        s = RE.config_from_chunks(eng.get_config().s[0], X.N)
    ref = []
    rec = lambda it, s_, acc, E: ref.append((it, RE.chunks_from_config(s_), acc, E)) or True
    if sampler == "rrr":
        AF.AfRun(AF.reference_of(X), s, beta, seed, oracle, replica=0).run(iters, step, hook=rec)
    else:
        AF.standard_mc(AF.reference_of(X), s, beta, iters, step, seed, oracle, replica=0, hook=rec)
    assert len(ref) == len(seen)
    for (it, cfg, acc, E), (rit, rs, racc, rE) in zip(seen, ref):
        assert it == rit and (cfg[0] == rs).all() and acc[0] == racc and E[0] == rE


@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_a_replica_stops_when_its_hook_returns_false(pkg, sampler):
    beta, iters, step, R, seed = 1.0, 600, 100, 3, 5
    X = wrap(pkg, 1, "sat33")
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=seed, quiet=True, replicas=R)
    at = {}

    def hook(it, X_, Cfg, acc, E):
        if it == 300:
            at["s"] = Cfg.s[1].copy()
        return np.array([True, it < 300, True])

    Es1, C1 = run(X, beta, iters, step=step, seed=seed, quiet=True, replicas=R, hook=hook)
    assert len(Es1[0]) == 6 and len(Es1[1]) == 3 and len(Es1[2]) == 6
    assert list(Es1[1]) == list(np.asarray(Es0)[1][:3]) and list(Es1[0]) == list(np.asarray(Es0)[0])
    assert (C1.s[1] == at["s"]).all() and (C1.s[0] == C0.s[0]).all() and (C1.s[2] == C0.s[2]).all()
