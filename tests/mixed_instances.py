"""The GraphMixed instances of the GPU tests, the smallest that reach each hazard, and the helpers that run them on the engine and hold
the result to the restatement (tests/mixed_reference.py) bit for bit.  TEST INFRASTRUCTURE."""
import os

import numpy as np

import add_fields_reference as AF
import mixed_reference as MR
import re_reference as RE
import sat_reference as SR

SEED = 190417
THREAD, WAVE = 1, 2


def ragged_sat65(pkg):
    """65 variables: a unit clause, an isolated variable (64), and variable 0 in 70 clauses (two ballot passes of the wave build)"""
    A, J = [[0]], [[1]]
    rng = np.random.default_rng(65)
    for a in range(69):
        others = sorted(int(x) for x in rng.choice(np.arange(1, 64), 2, replace=False))
        A.append([0] + others)
        J.append([int(b) for b in rng.integers(0, 2, 3)])
    for a in range(40):
        vs = sorted(int(x) for x in rng.choice(np.arange(1, 64), 3, replace=False))
        A.append(vs)
        J.append([int(b) for b in rng.integers(0, 2, 3)])
    return pkg.GraphSAT.from_clauses(65, A, J)


def mix(pkg, name):
    if name == "odd15":          # all six storage groups; GraphPercStep(15, 70) has two 64-pattern mask words
        return pkg.GraphMixed(pkg.GraphSK(15, seed=1), pkg.GraphSKNormal(15, seed=2), pkg.GraphPercStep(15, 70, seed=3), pkg.GraphCommStep(3, 5, 7, seed=4),
                              pkg.GraphSAT(15, 3, 4.2, seed=5), pkg.GraphRRGNormal(15, 4, seed=6))
    if name == "even8":          # GraphEANormal(2, 3): every bond doubled, K = 6
        return pkg.GraphMixed(pkg.GraphEANormal(2, 3, seed=7), pkg.GraphCommReLU(2, 4, 5, seed=8), pkg.GraphSK(8, seed=9), None)
    if name == "n65":            # three spin words, two passes of the lane-strided GraphSKNormal update
        return pkg.GraphMixed(pkg.GraphPercLinear(65, 3, seed=10), ragged_sat65(pkg), pkg.GraphSKNormal(65, seed=11), pkg.GraphRRG(65, 4, seed=12))
    if name == "xentr33":
        return pkg.GraphMixed(pkg.GraphPercXEntr(33, 5, 0.8, seed=13), pkg.GraphSK(33, seed=14))
    if name == "int21":          # every Es is an exact integer
        return pkg.GraphMixed(pkg.GraphSAT(21, 3, 3.0, seed=15), pkg.GraphPercStep(21, 9, seed=16))
    if name == "order-a":
        return pkg.GraphMixed(pkg.GraphSKNormal(15, seed=2), pkg.GraphSK(15, seed=1), pkg.GraphRRGNormal(15, 4, seed=6))
    if name == "order-b":
        return pkg.GraphMixed(pkg.GraphRRGNormal(15, 4, seed=6), pkg.GraphSK(15, seed=1), pkg.GraphSKNormal(15, seed=2))
    raise KeyError(name)


def fields(N, seed=5):
    h = np.random.default_rng(seed).normal(size=N)
    h[0] = 0.0
    h[N // 2] = -0.0
    return h


class forced:
    """force a standardMC build (RRRMC_MIXED_NO_WAVE / RRRMC_MIXED_WAVE) or an rrrMC build (RRRMC_AF_NO_LDS) for the block"""
    NAMES = ("RRRMC_MIXED_NO_WAVE", "RRRMC_MIXED_WAVE", "RRRMC_AF_NO_LDS")

    def __init__(self, std_build=None, af_build=None):
        self.set = {}
        if std_build == THREAD:
            self.set["RRRMC_MIXED_NO_WAVE"] = "1"
        if std_build == WAVE:
            self.set["RRRMC_MIXED_WAVE"] = "1"
        if af_build == 2:
            self.set["RRRMC_AF_NO_LDS"] = "1"

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.NAMES}
        os.environ.update(self.set)

    def __exit__(self, *a):
        for k in self.NAMES:
            os.environ.pop(k, None)
            if self.old[k] is not None:
                os.environ[k] = self.old[k]


def run_standard(pkg, X, R, beta, pieces, step, build=None, devices=None, debug=True):
    with forced(std_build=build), pkg.Engine(X, R, devices=devices) as eng:
        eng.set_debug_checks(debug)
        eng.seed(SEED)
        eng.init_spins_random()
        assert eng.mixed_build() == 0
        C0 = eng.get_config()
        E0 = np.atleast_1d(eng.energy())
        parts0 = np.atleast_2d(eng.mixed_energies())
        Es, acc = [], np.zeros(R, np.int64)
        for k, n in enumerate(pieces):
            eng.set_resume(k > 0)
            e, a = eng.standard_mc(beta, n, step)
            Es.append(np.atleast_2d(e).reshape(R, -1))
            acc += a
            if build is not None:
                assert eng.mixed_build() == build
        eng.set_resume(False)
        return dict(C0=C0, E0=E0, parts0=parts0, Es=np.concatenate(Es, axis=1), acc=acc, C1=eng.get_config(), Etr=np.atleast_1d(eng.run_energy()),
                    parts1=np.atleast_2d(eng.mixed_energies()), build=eng.mixed_build())


def check_standard(oracle, X, out, R, beta, iters, step, replicas=None):
    """Es, accepted counts, final spins, the tracked E and the components' energies against the restatement: no tolerances"""
    chains = {}
    for r in sorted((replicas or {0, R - 1}) & set(range(R))):
        s = RE.config_from_chunks(out["C0"].s[r], X.N)
        ref = MR.as_chain(X)
        assert float(out["E0"][r]) == float(ref.energy(s.copy())), r
        mixed = ref.g                                       # the Mixed under the (possibly zero) fields: its undo-path counters
        assert [float(x) for x in out["parts0"][r]] == [float(e) for e in MR.reference_of(X.X1 if hasattr(X, "X1") else X).energies(s.copy())], r
        es, E, a = AF.standard_mc(ref, s, beta, iters, step, SEED, oracle, replica=r)
        assert out["Es"][r].tolist() == [float(x) for x in es], r
        assert out["acc"][r] == a and float(out["Etr"][r]) == float(E), r
        assert (out["C1"].s[r] == RE.chunks_from_config(s)).all(), r
        chains[r] = mixed
    return chains


def run_rrr(pkg, X, R, beta, thr, af_build, pieces, step, devices=None):
    with forced(af_build=af_build), pkg.Engine(X, R, devices=devices) as eng:
        eng.set_debug_checks(True)
        eng.seed(SEED)
        eng.init_spins_random()
        assert eng.af_build() == 0
        C0 = eng.get_config()
        E0 = np.atleast_1d(eng.energy())
        Es, acc, st = [], np.zeros(R, np.int64), np.zeros(R, np.int64)
        for k, n in enumerate(pieces):
            eng.set_resume(k > 0)
            e, a, s = eng.rrr_mc(beta, n, step, staged_thr=thr)
            Es.append(np.atleast_2d(e).reshape(R, -1))
            acc += a
            st += s
            assert eng.af_build() == af_build
        eng.set_resume(False)
        return dict(C0=C0, E0=E0, Es=np.concatenate(Es, axis=1), acc=acc, staged=st, C1=eng.get_config(), Etr=np.atleast_1d(eng.run_energy()),
                    cache=eng.af_cache())


def check_rrr(oracle, X, out, R, beta, thr, iters, step, replicas=None):
    for r in sorted((replicas or {0, R - 1}) & set(range(R))):
        s = RE.config_from_chunks(out["C0"].s[r], X.N)
        run = AF.AfRun(MR.reference_of(X), s, beta, SEED, oracle, replica=r, staged_thr=thr)
        assert out["E0"][r] == run.E, r
        es = run.run(iters, step)
        assert out["Es"][r].tolist() == es, r
        assert out["acc"][r] == run.accepted and out["staged"][r] == run.staged_its, r
        assert (out["C1"].s[r] == RE.chunks_from_config(s)).all(), r
        assert out["Etr"][r] == run.E, r
        dEs, v, z, tref = run.cache_view()
        assert out["cache"][0][r].tolist() == dEs and out["cache"][1][r].tolist() == v, r          # af_cache equal to its definition
        assert out["cache"][2][r] == z and out["cache"][3][r] == tref, r
        assert all(v[i] == run.prior(beta * dEs[i]) and dEs[i] == run.X.delta0(s, i) for i in range(X.N))
    return run
