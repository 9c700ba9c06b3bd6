"""Hooks and resumed calls on the Robust Ensemble (DESIGN §4j applied to src/graphs/RE.jl): a hooked run is the un-hooked run, a run cut into
resumed calls anywhere is the run made in one call, a stopping hook ends the chain where the reference does, REenergies(X) inside the hook
is the sample's, a two-shard context equals the single one, and examples/test_reising.py writes its log."""
import os
import subprocess
import sys

import numpy as np
import pytest

import re_reference as RE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _skn(pkg, Nk, M):
    return pkg.GraphRobustEnsemble(Nk, M, 1.5, 2.0, pkg.GraphSKNormal(Nk, seed=17))


@pytest.mark.parametrize("kind", ["sk", "skn"])
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hooked_run_equals_unhooked_and_reenergies_in_hook(pkg, oracle, kind, sampler):
    Nk, M, beta, iters, step, R = 12, 5, 1.3, 4000, 100, 3
    X = pkg.GraphSKRE(Nk, M, 1.5, 2.0, seed=23) if kind == "sk" else _skn(pkg, Nk, M)
    J = X.J
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    seen = []

    def hook(it, X_, Cfg, acc, E):
        REs = pkg.REenergies(X_)
        assert REs.shape == (R, M)
        for r in range(R):
            s = RE.config_from_chunks(Cfg.s[r], X_.N)
            assert REs[r].tolist() == RE.re_energies(Nk, M, kind, J, s)
        seen.append(it)
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all()
    assert (C0.s == C1.s).all()


def test_reenergies_single_replica_shape(pkg):
    X = pkg.GraphSKRE(16, 4, 1.0, 1.0, seed=5)
    shapes = []
    pkg.rrrMC(X, 1.0, 300, step=100, seed=3, quiet=True, hook=lambda it, X_, C_, a, E: shapes.append(pkg.REenergies(X_).shape) or True)
    assert shapes == [(4,)] * 3


@pytest.mark.parametrize("kind", ["empty", "sk", "skn"])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, kind):
    Nk, M, R, beta, step, total = 9, 6, 4, 1.1, 50, 3000
    X = pkg.Graph0RE(Nk, M, 1.5, 2.0) if kind == "empty" else pkg.GraphSKRE(Nk, M, 1.5, 2.0, seed=4) if kind == "sk" else _skn(pkg, Nk, M)
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
    X = pkg.GraphSKRE(Nk, M, 1.5, 2.0, seed=8)
    calls = []
    Es, Cfg = pkg.rrrMC(X, beta, 5000, step=step, seed=19, quiet=True, hook=lambda it, *a: (calls.append(it), it < 700)[1])
    assert calls == list(range(100, 800, 100)) and len(Es[0]) == 7
    # the restatement stops at the same sample: the configuration is the one the hook saw at it = 700
    X2 = RE.make_ensemble(Nk, M, 1.5, 2.0, "sk", X.J)
    s = RE.config_from_chunks(oracle.init_config(19, 0, Nk * M), Nk * M)
    run = RE.RrrRun(X2, s, beta, 19, oracle)
    es = run.run(5000, step, hook=lambda it, s_, acc, E: it < 700)
    assert np.asarray(Es[0]).tolist() == es
    assert (Cfg.s[0] == RE.chunks_from_config(s)).all()


@pytest.mark.parametrize("kind", ["empty", "sk"])
def test_two_shard_context_equals_single(pkg, kind):
    X = pkg.Graph0RE(20, 5, 2.0, 0.4) if kind == "empty" else pkg.GraphSKRE(20, 5, 2.0, 0.4, seed=2)
    res = []
    for devices in (None, [0, 0]):
        with pkg.Engine(X, 70, devices=devices) as eng:
            eng.seed(5)
            eng.init_spins_random()
            r1 = eng.rrr_mc(0.4, 3000, 100)
            r2 = eng.standard_mc(0.4, 3000, 100)
            res.append((r1, r2, eng.get_config().s.copy(), eng.re_energies()))
    (a1, a2, ca, ra), (b1, b2, cb, rb) = res
    for x, y in zip(a1 + a2, b1 + b2):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert (ca == cb).all() and (ra == rb).all()


def test_debug_checks_pass_on_a_run(pkg):
    X = _skn(pkg, 8, 4)
    with pkg.Engine(X, 3) as eng:
        eng.set_debug_checks(True)
        eng.seed(2)
        eng.init_spins_random()
        eng.rrr_mc(1.0, 2000, 100)
        eng.standard_mc(1.0, 2000, 100)
        tot, sw, nl = eng.last_timing()
        assert nl == 1 and sw > 0


def test_example_writes_header_and_rows(tmp_path):
    out = str(tmp_path / "re")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "test_reising.py"), "--N", "64", "--step", "200", "--samples", "5",
                        "--t-limit", "60", "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = sorted(os.listdir(out))
    assert len(files) == 2
    for f in files:
        lines = open(os.path.join(out, f)).read().splitlines()
        assert lines[0] == "#mctime acc meanRE clocktime E"
        assert len(lines) == 6
        assert all(len(l.split()) == 5 for l in lines[1:])
