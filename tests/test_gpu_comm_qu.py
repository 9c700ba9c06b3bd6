"""GPU parity for the third binary committee machine (src/graphs/CommQu.jl): standardMC on the stand-alone GraphCommQu, rrrMC / standardMC
on GraphCommQuRE / GraphCommQuLE and on GraphQCommQuT, equal the plain-Python restatement (tests/comm_qu_reference.py composed with
re_reference / le_reference / quant_pattern_reference) bit for bit, with the debug checks on; a shape whose Δ2 passes int16; the kernel
builds, hooked and resumed runs and two-shard contexts agree; refusals on live contexts; and the final configurations of many chains follow
exp(-β E) / Z exactly (χ², energies from the definition)."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import comm_qu_reference as QR
import le_reference as LE
import quant_pattern_reference as QP
import re_reference as RE
from test_gpu_comm import _chi2, _state_index, _wilson_hilferty_limit
from test_gpu_quant_pattern_parity import _observables_from_definition

pytestmark = pytest.mark.gpu

RUNTESTS = [(24, 6, 30, False), (22, 6, 30, True)]                                   # test/runtests.jl:76-77
# a mask-word edge on each side (64, 65), one pattern, units that straddle a 32-bit spin word (K1 = 22, 24; 6), three mask words
SHAPES = RUNTESTS + [(2, 2, 1, False), (4, 4, 64, False), (6, 2, 65, False), (2, 4, 129, True)]
SWITCHES = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS", "RRRMC_LE_NO_LDS", "RRRMC_LE_LDS", "RRRMC_QUANT_NO_WAVE", "RRRMC_QUANT_NO_LDS", "RRRMC_QUANT_WAVE_MAX_R")


class _env:
    """the build switches of `env` for the duration of a block, every other one unset"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _graph(pkg, ens, K1, K2, P, M, gamma, beta_g, seed, fc=False):
    X1 = pkg.GraphCommQu(K1, K2, P, fc=fc, seed=seed)
    return {"re": pkg.GraphCommQuRE, "le": pkg.GraphCommQuLE}[ens](X1, M, gamma, beta_g), X1


def _ref(ens, X1, M, gamma, beta_g):
    return (QR.re_ensemble if ens == "re" else QR.le_ensemble)(X1.K2, X1.patterns(), X1.labels(), M, gamma, beta_g)


def _slice_energies(X1, rows, s):
    return [float(QR.energy_from_definition(X1.K2, X1.patterns(), X1.labels(), np.asarray(s[k::rows], np.int64))) for k in range(rows)]


def _check_observables(eng, ens, R, X1, M, configs):
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
        assert np.asarray(D if R == 1 else D[r]).tolist() == LE.distances(X1.N, M, s)


# ---- the stand-alone graph --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 1.1, 40.0])
@pytest.mark.parametrize("K1,K2,P,fc", SHAPES)
def test_standalone_standard_mc_bit_exact(pkg, oracle, K1, K2, P, fc, beta):
    seed, R, iters, step = 913 + K1 * K2, 3, 1000, 100
    X = pkg.GraphCommQu(K1, K2, P, fc=fc, seed=seed)
    xi, y = X.patterns(), X.labels()
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        E0 = eng.energy()
        assert E0.dtype == X.energy_dtype
        Es, acc = eng.standard_mc(beta, iters, step)
        Es2, acc2 = eng.standard_mc(beta, iters, step)          # a second call continues the streams
        C1 = eng.get_config()
        Etr = eng.run_energy()
        for r in range(R):
            s = RE.config_from_chunks(C0.s[r], X.N)
            assert E0[r] == QR.make(K2, xi, y).energy(s) == QR.energy_from_definition(K2, xi, y, s)
            es, E, a = QR.standard_mc(QR.make(K2, xi, y), s, beta, iters, step, seed, oracle, replica=r)
            assert Es[r].tolist() == es and acc[r] == a
            es, E, a = QR.standard_mc(QR.make(K2, xi, y), s, beta, iters, step, seed, oracle, replica=r, it0=iters)
            assert Es2[r].tolist() == es and acc2[r] == a
            assert (C1.s[r] == RE.chunks_from_config(s)).all()
            assert Etr[r] == E == QR.energy_from_definition(K2, xi, y, s)


def test_delta2_beyond_int16(pkg, oracle):
    """K1 = 130, K2 = 4, P = 2: the start equals pattern 0 on units 0 and 1 and is at Hamming distance 65 from it on units 2 and 3, so
    Δ1 = (130, 130, 0, 0) and Δ2[0] = ±2 · 130² = ±33 800: a 16-bit Δ2 would wrap"""
    K1, K2, beta, iters, step, seed = 130, 4, 2.0, 2000, 100, 77
    rng = np.random.default_rng(5)
    xi = rng.integers(0, 2, (2, K1 * K2))
    s0 = xi[0].copy()
    for u in (2, 3):
        s0[u * K1:u * K1 + 65] ^= 1
    for y in ([1, 0], [0, 1]):
        X = pkg.GraphCommQu.from_patterns(K2, xi, np.array(y))
        ref = QR.make(K2, xi, y)
        s = s0.copy()
        assert ref.energy(s) == QR.energy_from_definition(K2, xi, y, s) and ref.d2[0] == (33800 if y[0] else -33800)
        with pkg.Engine(X, 2) as eng:
            eng.set_debug_checks(True)
            eng.seed(seed)
            eng.set_config(pkg.Config(X.N, 2, np.stack([RE.chunks_from_config(s0)] * 2)))
            assert eng.energy().tolist() == [ref.energy(s)] * 2
            Es, acc = eng.standard_mc(beta, iters, step)
            eng.sync()                                           # the debug check reports here
            C1, Etr = eng.get_config(), eng.run_energy()
            for r in range(2):
                s = s0.copy()
                es, E, a = QR.standard_mc(QR.make(K2, xi, y), s, beta, iters, step, seed, oracle, replica=r)
                assert Es[r].tolist() == es and acc[r] == a and Etr[r] == E == QR.energy_from_definition(K2, xi, y, s)
                assert (C1.s[r] == RE.chunks_from_config(s)).all()


def test_standalone_resumed_sharded_and_hooked(pkg):
    X = pkg.GraphCommQu(6, 4, 80, seed=9)
    with pkg.Engine(X, 70) as a, pkg.Engine(X, 70) as b, pkg.Engine(X, 70, devices=[0, 0]) as c:
        for e in (a, b, c):
            e.set_debug_checks(True)
            e.seed(31)
            e.init_spins_random()
        Ea, acca = a.standard_mc(0.9, 3000, 50)
        Ec, accc = c.standard_mc(0.9, 3000, 50)
        b.set_resume(True)
        acc = np.zeros(70, np.int64)
        for n in (350, 1, 1649, 1000):
            acc += b.standard_mc(0.9, n, 50)[1]
        assert (acca == acc).all() and (acca == accc).all() and (Ea == Ec).all()
        assert (a.get_config().s == b.get_config().s).all() and (a.get_config().s == c.get_config().s).all()
        assert (a.run_energy() == b.run_energy()).all() and (a.energy() == c.energy()).all()
    Es0, C0 = pkg.standardMC(X, 0.9, 2000, step=100, seed=5, quiet=True, replicas=3)
    Es1, C1 = pkg.standardMC(X, 0.9, 2000, step=100, seed=5, quiet=True, replicas=3, hook=lambda *a: True)
    assert (np.asarray(Es0) == np.asarray(Es1)).all() and (C0.s == C1.s).all()


# ---- the ensembles ---------------------------------------------------------------------------------------------------------------
def _check_rrr(pkg, oracle, ens, K1, K2, P, M, gamma, beta_g, beta, R, iters, step, thr, fc=False, check_reps=None, calls=1):
    seed = 51301 + 31 * K1 * K2 + M
    X, X1 = _graph(pkg, ens, K1, K2, P, M, gamma, beta_g, seed, fc)
    N = X.N
    Ref = RE if ens == "re" else LE
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        E0 = eng.energy()
        outs = []
        for c in range(calls):          # a second call continues the streams (not the run: resume is off)
            Es, acc, staged = eng.rrr_mc(beta, iters, step, staged_thr=thr)
            outs.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config(), eng.rrr_cache(), eng.run_energy()))
        finals = {}
        Ef = eng.energy()
        for r in (check_reps if check_reps is not None else range(R)):
            s = Ref.config_from_chunks(C0.s[r], N)
            assert E0[r] == _ref(ens, X1, M, gamma, beta_g).energy(np.array(s, np.int64))
            for c in range(calls):
                run = Ref.RrrRun(_ref(ens, X1, M, gamma, beta_g), s, beta, seed, oracle, replica=r, it0=c * iters, staged_thr=thr)
                es = run.run(iters, step)
                Es, acc, staged, C1, (pos, sizes), Etr = outs[c]
                assert np.asarray(Es[r]).tolist() == es, (r, c)
                assert acc[r] == run.accepted and staged[r] == run.staged_its, (r, c)
                assert (C1.s[r] == Ref.chunks_from_config(s)).all(), (r, c)
                p_ref, sz_ref = run.cache_view()
                assert (pos[r] == p_ref).all() and (sizes[r] == sz_ref).all(), (r, c)
                assert Etr[r] == run.E
            assert Ef[r] == _ref(ens, X1, M, gamma, beta_g).energy(np.array(s, np.int64))
            finals[r] = s
        _check_observables(eng, ens, R, X1, M, finals.items())


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("K1,K2,P,fc", RUNTESTS)
def test_rrr_ensembles_runtests_shapes_bit_exact(pkg, oracle, ens, K1, K2, P, fc):
    # test/runtests.jl:100-101, 112-113: M = 5, γ = 0.5, β = 2.0
    _check_rrr(pkg, oracle, ens, K1, K2, P, 5, 0.5, 2.0, 2.0, 2, 2000, 100, 0.5, fc=fc)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("thr", [0.0, 1.0])
def test_rrr_ensembles_staged_thresholds(pkg, oracle, ens, thr):
    _check_rrr(pkg, oracle, ens, 4, 2, 40, 5, 1.5, 2.0, 1.2, 3, 3000, 100, thr)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("K1,K2,P,M,R", [(2, 4, 129, 6, 2), (2, 4, 129, 6, 3), (4, 2, 7, 7, 70)])
def test_rrr_ensembles_odd_even_M_many_replicas(pkg, oracle, ens, K1, K2, P, M, R):
    _check_rrr(pkg, oracle, ens, K1, K2, P, M, 0.7, 1.0, 1.3, R, 2500, 250, 0.5, check_reps=[0, 1, R - 1] if R > 3 else None, calls=2)


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("K1,K2,P,fc,M", [RUNTESTS[0] + (5,), RUNTESTS[1] + (5,), (4, 2, 70, False, 4)])
def test_standard_ensembles_bit_exact(pkg, oracle, ens, K1, K2, P, fc, M):
    gamma, beta_g, beta, R = 0.5, 2.0, 1.2, 3
    seed = 5511 + M + K1
    X, X1 = _graph(pkg, ens, K1, K2, P, M, gamma, beta_g, seed, fc)
    Ref = RE if ens == "re" else LE
    with pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        outs = [eng.standard_mc(beta, 2000, 100) + (eng.get_config(), eng.run_energy()) for _ in range(2)]
        finals = []
        for r in range(R):
            s = Ref.config_from_chunks(C0.s[r], X.N)
            for c, (Es, acc, C1, Etr) in enumerate(outs):
                es, E, a = Ref.standard_mc(_ref(ens, X1, M, gamma, beta_g), s, beta, 2000, 100, seed, oracle, replica=r, it0=2000 * c)
                assert Es[r].tolist() == es and acc[r] == a
                assert (C1.s[r] == Ref.chunks_from_config(s)).all()
                assert Etr[r] == E
            finals.append((r, s))
        _check_observables(eng, ens, R, X1, M, finals)


@pytest.mark.parametrize("ens", ["re", "le"])
def test_lds_and_thread_builds_agree(pkg, ens):
    X, _ = _graph(pkg, ens, 6, 4, 130, 6, 1.2, 1.0, 3)
    up = ens.upper()

    def run(env):
        with _env(env), pkg.Engine(X, 37) as eng:
            eng.set_debug_checks(True)
            eng.seed(99)
            eng.init_spins_random()
            out = eng.rrr_mc(1.7, 5000, 50) + eng.rrr_mc(1.7, 3000, 50, staged_thr=1.0)
            return out, eng.get_config().s.copy(), eng.rrr_cache()

    (a, ca, pa), (b, cb, pb) = run({"RRRMC_%s_NO_LDS" % up: "1"}), run({"RRRMC_%s_LDS" % up: "1"})
    for x, y in zip(a, b):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert (ca == cb).all() and (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()


def _lds_bytes(ens, K1, K2, P, M, qu=True):
    """the dynamic LDS of the LDS build of rrrMC: re_rrr_lds_bytes / le_rrr_lds_bytes (csrc/re_kernels.hpp, csrc/le_kernels.hpp) plus
    comm_lds_bytes (csrc/comm_kernels.hpp).  qu = False: what the rows of a step / ReLU machine of that shape would take"""
    Nk, rows = K1 * K2, M if ens == "re" else M + 1
    N, PW = Nk * rows, (P + 63) // 64
    W = 2 * ((N + 63) // 64)
    base = W * 4 + ((N * 2 + 3) & ~3) + ((N + 3) & ~3) + ((Nk + 3) & ~3) + (32 * 4 if ens == "re" else 2 * 17 * 4) + 64 * 8 * 4
    row = 2 * 8 + (K2 + 2) * 64 * 2 if qu else (2 * K2 + 2) * 8 + (K2 + 1) * 64 * 2
    return ((base + 7) & ~7) + rows * PW * row


LDS_LIMIT = 160 * 1024
# (ens, the largest P of GraphCommQu(32, 4, P) x 5 whose rows fit, the next mask word: it does not)
LARGEST = [("re", 2560, 2624), ("le", 2112, 2176)]


@pytest.mark.parametrize("ens,fits,too_big", LARGEST)
def test_largest_shapes_lds_when_the_qu_rows_fit_thread_build_when_not(pkg, ens, fits, too_big):
    """The LDS build is sized with the Qu row (32-bit Δ2, two mask words): 784 bytes per slice and mask word at K2 = 4, where a ReLU row
    takes 720.  `fits` runs in both builds; `too_big` passes 160 KB only with the Qu row size (with the ReLU size it would be launched in
    the LDS build and overrun it), runs without a switch — in the thread build — and equals the thread build asked for, even when the LDS
    build is asked for.  Tracked energy against a fresh one, debug checks on."""
    K1, K2, M = 32, 4, 5
    assert _lds_bytes(ens, K1, K2, fits, M) <= LDS_LIMIT < _lds_bytes(ens, K1, K2, too_big, M)
    assert _lds_bytes(ens, K1, K2, too_big, M, qu=False) <= LDS_LIMIT
    up = ens.upper()
    no_lds, lds = {"RRRMC_%s_NO_LDS" % up: "1"}, {"RRRMC_%s_LDS" % up: "1"}
    for P, envs in ((fits, (no_lds, lds, {})), (too_big, (no_lds, {}, lds))):
        X, _ = _graph(pkg, ens, K1, K2, P, M, 1.0, 2.0, 2)
        runs = []
        for env in envs:
            with _env(env), pkg.Engine(X, 2) as eng:
                eng.set_debug_checks(True)
                eng.seed(4)
                eng.init_spins_random()
                out = eng.rrr_mc(2.0, 1500, 500)
                Etr, E = eng.run_energy(), eng.energy()
                assert (np.abs(Etr - E) <= 1e-10 * np.maximum(1.0, np.abs(E))).all()
                runs.append(out + (eng.get_config().s.copy(),) + eng.rrr_cache())
        for other in runs[1:]:
            for x, y in zip(runs[0], other):
                assert (np.asarray(x) == np.asarray(y)).all()


@pytest.mark.parametrize("ens", ["re", "le"])
@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_hooked_run_equals_unhooked_and_observables_in_hook(pkg, ens, sampler):
    M, beta, iters, step, R = 5, 1.3, 2000, 100, 3
    X, X1 = _graph(pkg, ens, 4, 2, 40, M, 1.5, 2.0, 23)
    run = pkg.rrrMC if sampler == "rrr" else pkg.standardMC
    Es0, C0 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R)
    seen = []

    def hook(it, X_, Cfg, acc, E):
        rows = M if ens == "re" else M + 1
        obs = pkg.REenergies(X_) if ens == "re" else np.concatenate([pkg.cenergy(X_)[:, None], pkg.LEenergies(X_)], axis=1)
        assert obs.shape == (R, rows)
        for r in range(R):
            s = RE.config_from_chunks(Cfg.s[r], X_.N)
            assert obs[r].tolist() == _slice_energies(X1, rows, s)          # the per-replica training error
            if ens == "le":
                assert pkg.distances(X_)[r].tolist() == LE.distances(X1.N, M, s)
        seen.append(it)
        return True

    Es1, C1 = run(X, beta, iters, step=step, seed=77, quiet=True, replicas=R, hook=hook)
    assert seen == list(range(step, iters + 1, step))
    assert (np.asarray(Es0) == np.asarray(Es1)).all()
    assert (C0.s == C1.s).all()


@pytest.mark.parametrize("ens", ["re", "le"])
def test_run_cut_into_resumed_calls_equals_one_call(pkg, ens):
    R, beta, step, total = 4, 1.1, 50, 3000
    X, _ = _graph(pkg, ens, 2, 4, 70, 6, 1.5, 2.0, 4)
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
def test_two_shard_ensemble_equals_single(pkg, ens):
    X, _ = _graph(pkg, ens, 6, 2, 70, 5, 2.0, 0.4, 2)
    res = []
    for devices in (None, [0, 0]):
        with pkg.Engine(X, 70, devices=devices) as eng:
            eng.seed(5)
            eng.init_spins_random()
            r1 = eng.rrr_mc(0.8, 3000, 100)
            cache = eng.rrr_cache()
            r2 = eng.standard_mc(0.8, 3000, 100)
            obs = (eng.re_energies(),) if ens == "re" else (eng.le_energies(), eng.cenergy(), eng.distances())
            res.append(r1 + r2 + cache + (eng.get_config().s.copy(), eng.energy()) + obs)
    for x, y in zip(*res):
        assert (np.asarray(x) == np.asarray(y)).all()


# ---- GraphQuant -------------------------------------------------------------------------------------------------------------------
Q_R, Q_ITERS, Q_STEP, Q_BETA, Q_SEED, Q_THR = 33, 600, 50, 1.5, 0xABCD, 0.55
# the three kernel builds and what Engine.quant_pattern_build reports: thread per replica (0), wavefront per replica with the slice state in
# HBM/L2 (1), wavefront per replica with it staged in LDS (2)
Q_BUILDS = {"thread": ({"RRRMC_QUANT_NO_WAVE": "1"}, 0), "wave-no-lds": ({"RRRMC_QUANT_NO_LDS": "1"}, 1), "lds": ({}, 2)}
Q_REPS = (0, 1, 32)                              # the replicas of a 33-replica run held to the reference (replica 0 is the R = 1 run)


def _qgraph(pkg, fc):
    K1, K2, P, _ = RUNTESTS[1] if fc else RUNTESTS[0]
    return pkg.GraphQCommQuT(K1, K2, P, 5, 0.5, 2.0, fc=fc, seed=17)                 # test/runtests.jl:88-89


@functools.lru_cache(maxsize=None)
def _qreference(pkg, oracle, fc):
    """the reference's run of a shape, both samplers, the replicas of Q_REPS: computed once, shared, never modified"""
    X = _qgraph(pkg, fc)
    out = {"rrr": {}, "std": {}}
    for r in Q_REPS:
        s = RE.config_from_chunks(oracle.init_configs(Q_SEED, r, 1, X.N)[0], X.N)
        ref = QR.quant_reference(X)
        run = QP.RrrRun(ref, s, Q_BETA, Q_SEED, oracle, replica=r, staged_thr=Q_THR)
        Es = run.run(Q_ITERS, Q_STEP)
        out["rrr"][r] = (Es, s.copy(), run.accepted, run.staged_its) + run.cache_view() + (run.E, ref.renergies())
        s = RE.config_from_chunks(oracle.init_configs(Q_SEED, r, 1, X.N)[0], X.N)
        ref = QR.quant_reference(X)
        Es, E, acc = QP.standard_mc(ref, s, Q_BETA, Q_ITERS, Q_STEP, Q_SEED, oracle, replica=r)
        out["std"][r] = (Es, s.copy(), acc, E, ref.renergies())
    return X, out


def _qrun(pkg, X, R, env, want):
    with _env(env), pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(Q_SEED)
        eng.init_spins_random()
        rrr = eng.rrr_mc(Q_BETA, Q_ITERS, Q_STEP, staged_thr=Q_THR)
        eng.sync()                                              # the debug mode reports here
        assert eng.quant_pattern_build() == want
        rrr += eng.rrr_cache() + (eng.get_config().s.copy(), eng.run_energy(), eng.quant_renergies()) + eng.quant_observables()
        eng.seed(Q_SEED)
        eng.init_spins_random()
        std = eng.standard_mc(Q_BETA, Q_ITERS, Q_STEP)
        assert eng.quant_pattern_build() == want
        std += (eng.get_config().s.copy(), eng.tracked_energy(), eng.quant_renergies())
    return rrr, std


@pytest.mark.parametrize("build,R", [("lds", 1), ("lds", 33), ("wave-no-lds", 1), ("wave-no-lds", 33), ("thread", 33)])
@pytest.mark.parametrize("fc", [False, True])
def test_quant_both_samplers_bit_identical_to_the_reference(pkg, oracle, fc, build, R):
    X, ref = _qreference(pkg, oracle, fc)
    rrr, std = _qrun(pkg, X, R, *Q_BUILDS[build])
    Es, acc, st, pos, sizes, cfg, Etr, ren, Q, tm, ov = rrr
    ren, ov, Q, tm = np.reshape(ren, (R, -1)), np.reshape(ov, (R, -1)), np.reshape(Q, R), np.reshape(tm, R)      # one replica: unbatched
    for r in [q for q in Q_REPS if q < R]:
        rEs, rs, racc, rst, rpos, rsizes, rE, rren = ref["rrr"][r]
        assert Es[r].tolist() == rEs and (cfg[r] == RE.chunks_from_config(rs)).all() and (acc[r], st[r]) == (racc, rst)
        assert (pos[r] == rpos).all() and (sizes[r] == rsizes).all() and Etr[r] == rE
        assert ren[r].tolist() == [float(e) for e in rren]
        assert rren == [QR.energy_from_definition(X.X1.K2, X.X1.patterns(), X.X1.labels(), rs[k * X.Nk:(k + 1) * X.Nk]) for k in range(X.M)]
        dQ, dtm, dov = _observables_from_definition(X, rs, rren)
        assert np.asarray(ov[r]).tolist() == dov
        assert abs(tm[r] - dtm) <= 1e-12 * abs(dtm) and abs(Q[r] - dQ) <= 1e-12 * abs(dQ)          # libm's cosh / sinh enter
    Es, acc, cfg, Etr, ren = std
    ren = np.reshape(ren, (R, -1))
    for r in [q for q in Q_REPS if q < R]:
        rEs, rs, racc, rE, rren = ref["std"][r]
        assert Es[r].tolist() == rEs and (cfg[r] == RE.chunks_from_config(rs)).all() and acc[r] == racc and Etr[r] == rE
        assert ren[r].tolist() == [float(e) for e in rren]


def test_quant_thread_build_at_2049_replicas_and_builds_continue_one_another(pkg, oracle):
    """2049 replicas, past the siblings' bound of the wave builds: for GraphCommQu slices it is 16 384 (profiles/r13/comm_qu.md), so the staged wave
    build runs unasked and the thread build when asked; both are bit for bit one another, and their first 33 replicas are the 33-replica run's
    (held to the reference above); a resumed run whose pieces go through the three builds in turn is the one-call run of the thread build"""
    X, ref = _qreference(pkg, oracle, False)
    big = _qrun(pkg, X, 2049, {"RRRMC_QUANT_NO_WAVE": "1"}, 0)
    wave = _qrun(pkg, X, 2049, {}, 2)
    small = _qrun(pkg, X, 33, {"RRRMC_QUANT_NO_WAVE": "1"}, 0)
    for sampler in (0, 1):
        for x, y, z in zip(big[sampler], wave[sampler], small[sampler]):
            assert (np.asarray(x) == np.asarray(y)).all() and (np.asarray(x)[:33] == np.asarray(z)).all()
    assert big[0][0][32].tolist() == ref["rrr"][32][0]
    R, total = 3, 900
    with _env({"RRRMC_QUANT_NO_WAVE": "1"}), pkg.Engine(X, R) as a:
        a.seed(31)
        a.init_spins_random()
        Ea, acca, sta = a.rrr_mc(Q_BETA, total, Q_STEP, staged_thr=Q_THR)
        Ca, pa = a.get_config().s.copy(), a.rrr_cache()
    with pkg.Engine(X, R) as b:
        b.set_debug_checks(True)
        b.seed(31)
        b.init_spins_random()
        b.set_resume(True)
        Es, acc, st, seen = [], np.zeros(R, np.int64), np.zeros(R, np.int64), []
        for n, env in ((217, {}), (301, {"RRRMC_QUANT_WAVE_MAX_R": str(R - 1)}), (149, {"RRRMC_QUANT_NO_LDS": "1"}), (233, {"RRRMC_QUANT_WAVE_MAX_R": str(R)})):
            with _env(env):
                e_, ac, s_ = b.rrr_mc(Q_BETA, n, Q_STEP, staged_thr=Q_THR)
            seen.append(b.quant_pattern_build())
            Es.append(e_)
            acc += ac
            st += s_
        assert seen == [2, 0, 1, 2]
        assert (Ea == np.concatenate(Es, axis=1)).all() and (acca == acc).all() and (sta == st).all()
        pb = b.rrr_cache()
        assert (Ca == b.get_config().s).all() and (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()


# ---- refusals on live contexts ----------------------------------------------------------------------------------------------------
def test_refusals_on_live_contexts(pkg):
    L = pkg.lib()
    X1 = pkg.GraphCommQu(2, 4, 5)
    with pkg.Engine(X1, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        xi = X1.xi.reshape(-1)
        assert L.rrrmc_set_comm_patterns(eng._ctx, 4, xi, None, 5) == 1                              # a missing y
        assert L.rrrmc_set_comm_patterns(eng._ctx, 6, xi, X1.y, 5) == 1                              # not the context's K2
        assert L.rrrmc_set_comm_patterns(eng._ctx, 4, xi, np.full(1, 32, np.uint64), 5) == 1         # a label bit beyond P
        assert L.rrrmc_set_comm_patterns(eng._ctx, 4, xi, X1.y, 5) == 0
        for call in (lambda: eng.rrr_mc(1.0, 100, 10), lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0),
                     lambda: eng.extremal_opt(1.4, 100, 10)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3
        eng.standard_mc(1.0, 100, 10)                                                                # and the context is still good
    for X in (pkg.GraphCommQuRE(2, 4, 5, 3, 1.0, 1.0), pkg.GraphCommQuLE(2, 4, 5, 3, 1.0, 1.0), pkg.GraphQCommQuT(2, 4, 5, 3, 1.0, 1.0)):
        with pkg.Engine(X, 2) as eng:
            eng.seed(1)
            eng.init_spins_random()
            for call in (lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0), lambda: eng.extremal_opt(1.4, 100, 10)):
                with pytest.raises(pkg.RRRMCError) as e:
                    call()
                assert e.value.code == 3
            eng.rrr_mc(1.0, 100, 10)
    ctx = C.c_void_p()
    for create in (L.rrrmc_ctx_create_re, L.rrrmc_ctx_create_le):
        assert create(C.byref(ctx), 8, 5, 9, 2, 0, 0) == 0
        assert L.rrrmc_set_comm_patterns(ctx, 2, np.zeros(3, np.uint64), None, 3) == 1               # a missing y
        assert L.rrrmc_set_comm_patterns(ctx, 1, np.zeros(3, np.uint64), np.zeros(1, np.uint64), 3) == 1      # K2 = 1 is odd
        assert L.rrrmc_set_comm_patterns(ctx, 4, np.zeros(3, np.uint64), np.zeros(1, np.uint64), 3) == 0      # K1 = 2, K2 = 4
        assert L.rrrmc_set_comm_patterns(ctx, 2, np.zeros(3, np.uint64), np.full(1, 8, np.uint64), 3) == 1    # a label bit beyond P
        assert L.rrrmc_set_comm_patterns(ctx, 2, np.zeros(3, np.uint64), np.zeros(1, np.uint64), 3) == 0
        assert L.rrrmc_set_patterns(ctx, np.zeros(3, np.uint64), 3) == 2                             # not a perceptron context
        L.rrrmc_ctx_destroy(ctx)
        assert create(C.byref(ctx), 8, 5, 7, 2, 0, 0) == 1                                           # kind 7 is still unassigned
        assert create(C.byref(ctx), 10, 5, 9, 2, 0, 0) == 1                                          # Nk % 4 != 0


# ---- the stationary distribution ---------------------------------------------------------------------------------------------------
QU_XI, QU_Y = [[1, 0, 0, 1, 1, 1, 0, 1], [0, 1, 1, 0, 1, 0, 0, 1]], [1, 0]        # CommQu(2, 4, P = 2): N = 8, 256 states
RE_XI, RE_Y = [[1, 0, 0, 1], [0, 1, 1, 1]], [1, 0]                                # RE(4, 3) over CommQu(2, 2, P = 2): N = 12, 4096 states
# at β = 0.6 the smallest expected count of the 4096 states at R = 65 536 is 3.2 (re_boltzmann_expected, no device needed); 0.5 gives 4.3 and
# 0.4 gives 5.8, the first that keeps every bin a valid χ² term
RE_BETA = 0.4


def test_standalone_final_configurations_follow_the_boltzmann_distribution(pkg):
    beta, R, K2 = 0.6, 65536, 4
    xi, y = np.array(QU_XI), np.array(QU_Y)
    X = pkg.GraphCommQu.from_patterns(K2, xi, y)
    N = X.N
    states = list(itertools.product((0, 1), repeat=N))
    E = np.array([QR.energy_from_definition(K2, xi, y, s) for s in states], np.float64)
    assert len(set(E.tolist())) > 1
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    expected = p * R
    # every bin a valid χ² term; guaranteed by R e^{-β (Emax - Emin)} / 2^N >= 5 (here 65 536 e^{-1.2} / 256 >= 77)
    assert R * np.exp(-beta * (E.max() - E.min())) / 2 ** N >= 5 and expected.min() >= 5
    with pkg.Engine(X, R) as eng:
        eng.seed(424242)
        eng.init_spins_random()
        eng.standard_mc(beta, 4000, 4000)
        idx = _state_index(eng.get_config(), N)
        assert (eng.run_energy() == E[idx]).all()
    stat = _chi2(np.bincount(idx, minlength=len(states)), expected)
    limit = _wilson_hilferty_limit(len(states) - 1)
    print("chi2 qu: %.1f (limit %.1f, smallest expected count %.1f)" % (stat, limit, expected.min()))
    assert stat < limit, (stat, limit)


def re_boltzmann_expected(R=65536, beta=RE_BETA):
    """(states, E, expected counts) of GraphRobustEnsemble(4, 3, γ = 0.6, β = 1.2) over CommQu(K1 = 2, K2 = 2, P = 2); no device needed"""
    Nk, M, gamma, beta_g = 4, 3, 0.6, 1.2
    xi, y = np.array(RE_XI), np.array(RE_Y)
    states = list(itertools.product((0, 1), repeat=Nk * M))

    def energy(s):                                 # -Σ_i log(2 cosh(γ μ_i)) / β + Σ_k E_k, E_k from the definition
        sg = 2 * np.asarray(s, np.int64).reshape(Nk, M) - 1
        E = -sum(np.log(2 * np.cosh(gamma * sg[i].sum())) / beta_g for i in range(Nk))
        return E + sum(QR.energy_from_definition(2, xi, y, (sg[:, k] + 1) // 2) for k in range(M))

    E = np.array([energy(s) for s in states])
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    return states, E, p * R


@pytest.mark.parametrize("sampler", ["rrr", "std"])
def test_ensemble_final_configurations_follow_the_boltzmann_distribution(pkg, sampler):
    Nk, M, gamma, beta_g, beta, R = 4, 3, 0.6, 1.2, RE_BETA, 65536
    X1 = pkg.GraphCommQu.from_patterns(2, np.array(RE_XI), np.array(RE_Y))
    X = pkg.GraphRobustEnsemble(Nk, M, gamma, beta_g, X1)
    N = X.N
    states, E, expected = re_boltzmann_expected(R, beta)
    assert expected.min() >= 5                     # every bin is a valid χ² term
    with pkg.Engine(X, R) as eng:
        eng.seed(424243)
        eng.init_spins_random()
        if sampler == "rrr":
            eng.rrr_mc(beta, 4000, 4000)
        else:
            eng.standard_mc(beta, 4000, 4000)
        idx = _state_index(eng.get_config(), N)
        assert np.abs(eng.run_energy() - E[idx]).max() < 1e-12
    stat = _chi2(np.bincount(idx, minlength=len(states)), expected)
    limit = _wilson_hilferty_limit(len(states) - 1)
    print("chi2 RE %s: %.1f (limit %.1f, smallest expected count %.1f)" % (sampler, stat, limit, expected.min()))
    assert stat < limit, (stat, limit)
