"""GPU parity for the Robust Ensemble and the Local Entropy ensemble over K-SAT slices (GraphSATRE / GraphSATLE, src/REAliases.jl:77-92,
src/LEAliases.jl:77-92): rrrMC and standardMC equal re_reference / le_reference composed with the literal ClauseCache of
tests/sat_reference.py bit for bit, in both kernel builds; REenergies / LEenergies / cenergy / distances are the configuration's; a
stopping hook freezes a replica where the reference stops; a run cut into resumed calls is the run made in one call."""
import os

import numpy as np
import pytest

import le_reference as LE
import re_reference as RE
import sat_reference as SR

pytestmark = pytest.mark.gpu

ENVS = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS", "RRRMC_LE_NO_LDS", "RRRMC_LE_LDS")
NK, K, ALPHA, M, GAMMA, BETA_G = 10, 3, 4.2, 3, 1.5, 2.0


def _graph(pkg, ens, seed=41):
    X1 = pkg.GraphSAT(NK, K, ALPHA, seed=seed)
    return (pkg.GraphSATRE if ens == "re" else pkg.GraphSATLE)(X1, M, GAMMA, BETA_G), X1


def _ref(ens, X1):
    return (SR.re_ensemble if ens == "re" else SR.le_ensemble)(NK, X1.A, X1.J, M, GAMMA, BETA_G)


def _slice_energies(X1, rows, s):
    return [float(SR.pure_energy(X1.A, X1.J, s[k::rows])) for k in range(rows)]


def _check_observables(eng, ens, R, X1, configs):
    if ens == "re":
        Es = eng.re_energies()
        for r, s in configs:
            assert np.asarray(Es if R == 1 else Es[r]).tolist() == _slice_energies(X1, M, s)
        return
    LEs, Ec, D = eng.le_energies(), eng.cenergy(), eng.distances()
    for r, s in configs:
        e = _slice_energies(X1, M + 1, s)
        assert np.asarray(LEs if R == 1 else LEs[r]).tolist() == e[1:]
        assert float(Ec if R == 1 else Ec[r]) == e[0]
        assert np.asarray(D if R == 1 else D[r]).tolist() == LE.distances(NK, M, s)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in ENVS}
    for k in ENVS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("thr", [0.0, None, 1.0])
@pytest.mark.parametrize("build", ["LDS", "NO_LDS"])
def test_rrr_bit_exact(pkg, oracle, ens, thr, build):
    seed, beta, R, iters, step = 9911, 1.2, 3, 3000, 100
    X, X1 = _graph(pkg, ens)
    Ref = RE if ens == "re" else LE

    def run():
        with pkg.Engine(X, R) as eng:
            eng.set_debug_checks(True)
            eng.seed(seed)
            eng.init_spins_random()
            C0 = eng.get_config()
            E0 = eng.energy()
            outs = []
            for c in range(2):              # a second call continues the streams (not the run: resume is off)
                Es, acc, staged = eng.rrr_mc(beta, iters, step, staged_thr=thr)
                outs.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config(), eng.rrr_cache(), eng.run_energy()))
            finals = {}
            for r in range(R):
                s = Ref.config_from_chunks(C0.s[r], X.N)
                assert E0[r] == _ref(ens, X1).energy(np.array(s, np.int64))
                for c in range(2):
                    rr = Ref.RrrRun(_ref(ens, X1), s, beta, seed, oracle, replica=r, it0=c * iters, staged_thr=0.5 if thr is None else thr)
                    es = rr.run(iters, step)
                    Es, acc, staged, C1, (pos, sizes), Etr = outs[c]
                    assert np.asarray(Es[r]).tolist() == es, (r, c)
                    assert acc[r] == rr.accepted and staged[r] == rr.staged_its, (r, c)
                    assert (C1.s[r] == Ref.chunks_from_config(s)).all(), (r, c)
                    p_ref, sz_ref = rr.cache_view()
                    assert (pos[r] == p_ref).all() and (sizes[r] == sz_ref).all(), (r, c)
                    assert Etr[r] == rr.E
                finals[r] = s
            _check_observables(eng, ens, R, X1, finals.items())

    up = ens.upper()
    _with_env({"RRRMC_%s_%s" % (up, build): "1"}, run)


@pytest.mark.parametrize("ens", ["re", "le"])
def test_standard_bit_exact(pkg, oracle, ens):
    seed, beta, R = 5513, 1.2, 3
    X, X1 = _graph(pkg, ens)
    Ref = RE if ens == "re" else LE
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        Es, acc = eng.standard_mc(beta, 3000, 100)
        C1 = eng.get_config()
        Etr = eng.run_energy()
        finals = []
        for r in range(R):
            s = Ref.config_from_chunks(C0.s[r], X.N)
            es, E, a = Ref.standard_mc(_ref(ens, X1), s, beta, 3000, 100, seed, oracle, replica=r)
            assert Es[r].tolist() == es and acc[r] == a
            assert (C1.s[r] == Ref.chunks_from_config(s)).all()
            assert Etr[r] == E
            finals.append((r, s))
        _check_observables(eng, ens, R, X1, finals)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hook_sees_the_observables_and_stops_a_replica(pkg, ens, sampler):
    beta, iters, step, R = 1.3, 2000, 100, 3
    X, X1 = _graph(pkg, ens, seed=23)
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    rows = M if ens == "re" else M + 1
    seen = []

    def hook(it, X_, Cfg, acc, E):
        obs = pkg.REenergies(X_) if ens == "re" else np.concatenate([pkg.cenergy(X_)[:, None], pkg.LEenergies(X_)], axis=1)
        assert obs.shape == (R, rows)
        for r in range(R):
            s = RE.config_from_chunks(Cfg.s[r], X_.N)
            assert obs[r].tolist() == _slice_energies(X1, rows, s)
            if ens == "le":
                assert pkg.distances(X_)[r].tolist() == LE.distances(NK, M, s)
        seen.append(it)
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all() and (C0.s == C1.s).all()
    # replica 1 is stopped at it = 700: it keeps what it had then, the others run on as before
    Es2, C2 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=lambda it, *a: np.array([True, it < 700, True]))
    Es7, C7 = run(X, beta, 699, step=step, seed=77, quiet=True, replicas=R)
    for r in (0, 2):
        assert np.asarray(Es2[r]).tolist() == np.asarray(Es0[r]).tolist() and (C2.s[r] == C0.s[r]).all()
    assert np.asarray(Es2[1]).tolist()[:7] == np.asarray(Es0[1]).tolist()[:7] and len(Es2[1]) == 7
    assert (C2.s[1] == C7.s[1]).all()


@pytest.mark.parametrize("ens", ["re", "le"])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, ens):
    R, beta, step, total = 4, 1.1, 50, 3000
    X, _ = _graph(pkg, ens, seed=4)
    rng = np.random.default_rng(12)
    cuts = sorted(set(rng.integers(1, total, 7).tolist()))
    pieces = np.diff([0] + cuts + [total]).tolist()
    with pkg.Engine(X, R) as a, pkg.Engine(X, R) as b:
        for e in (a, b):
            e.set_debug_checks(True)
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
        assert (Ea == np.concatenate(Es, axis=1)).all() and (acca == acc).all() and (sta == st).all()
        assert (a.get_config().s == b.get_config().s).all()
        pa, pb = a.rrr_cache(), b.rrr_cache()
        assert (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
        assert (a.run_energy() == b.run_energy()).all()


@pytest.mark.parametrize("ens", ["re", "le"])
def test_two_shard_context_and_many_replicas(pkg, ens):
    X, _ = _graph(pkg, ens, seed=2)
    res = []
    for devices in (None, [0, 0]):
        with pkg.Engine(X, 70, devices=devices) as eng:
            eng.set_debug_checks(True)
            eng.seed(5)
            eng.init_spins_random()
            r1 = eng.rrr_mc(0.8, 2000, 100)
            cache = eng.rrr_cache()
            r2 = eng.standard_mc(0.8, 2000, 100)
            obs = (eng.re_energies(),) if ens == "re" else (eng.le_energies(), eng.cenergy(), eng.distances())
            res.append(r1 + r2 + cache + (eng.get_config().s.copy(),) + obs)
    for x, y in zip(*res):
        assert (np.asarray(x) == np.asarray(y)).all()
