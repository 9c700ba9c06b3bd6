"""The exact Boltzmann law on systems small enough to enumerate: what tests/test_gpu_boltzmann.py (the HIP library) and
tests/test_boltzmann_cpu.py (the CPU oracle) share.

Everything the parity tests trust was written by one author reading one reference: if library and oracle misread it in the same way, parity
holds and the physics is wrong.  Here the energies are written once more from the reference's `energy` definitions — numpy, Float64 or exact
integers, from the graph object's public arrays only — the 2^N states are enumerated, and the final configurations (or last sampled energies)
of many independent chains are scored against exp(-βE)/Z with a Pearson χ² whose limit is derived, not tuned.  A power check (the same counts
against the law at 1.1 β must FAIL the limit) shows that each case can tell a 10 % error in β.

A plain helper module: no fixture, no pytest setting.  Nothing here calls oracle.*_energy, Engine.energy() or tests/*_reference.py.
"""
import math
import os
from collections import namedtuple

import numpy as np


# ---- states -------------------------------------------------------------------------------------------------------------------------
def enumerate_states(N):
    """[2^N, N] array of 0/1: state `idx` has site 0 as its most significant bit (the order of itertools.product((0, 1), repeat=N))"""
    idx = np.arange(1 << N, dtype=np.int64)
    return ((idx[:, None] >> (N - 1 - np.arange(N))[None, :]) & 1).astype(np.int64)


def _state_index(Cfg, N):
    idx = np.zeros(Cfg.s.shape[0], np.int64)
    for j in range(N):                             # site 0 is the most significant bit, as itertools.product orders the states
        idx = idx * 2 + ((Cfg.s[:, 0] >> np.uint64(j)) & np.uint64(1)).astype(np.int64)
    return idx


def state_index_of_chunks(chunks, N):
    """_state_index for a bare [R, 1] array of chunks (what the oracle returns)"""
    return _state_index(namedtuple("C", "s")(np.ascontiguousarray(chunks, np.uint64).reshape(-1, 1)), N)


# ---- energies from the definition ---------------------------------------------------------------------------------------------------
def _sparse(A, J, sg):
    """-(1/2) Σ_x Σ_k J[x,k] σ_x σ_A[x,k]: the double loop of src/graphs/RRG.jl:164-189 (GraphRRG), EA.jl:195-222 (GraphEA; a bond listed
    twice, L = 2, counts twice), RRG.jl:532-559 (GraphRRGNormal) and EA.jl:584-611 (GraphEANormal).  `sg` is [S, N] of ±1; the result keeps J's
    arithmetic (exact integers for integer J)."""
    A = np.asarray(A, np.int64)
    n = np.zeros(sg.shape[0], J.dtype)
    for x in range(A.shape[0]):
        for k in range(A.shape[1]):
            n = n - J[x, k] * sg[:, x] * sg[:, A[x, k]]
    if np.issubdtype(J.dtype, np.integer):
        assert (n % 2 == 0).all()                  # every bond is listed from both ends (n /= 2 is exact: RRG.jl:185)
        return n // 2
    return n / 2


def energy_sparse_int(A, J, sg):
    """GraphRRG / GraphEA with integer couplings (RRG.jl:164-189, EA.jl:195-222): exact int64"""
    return _sparse(A, np.asarray(J, np.int64), sg)


def energy_sparse_levels(A, J, levels, sg):
    """GraphRRG{ET,LEV,K} with Int levels (RRG.jl:164-189): J holds level VALUES here (X.J are the values themselves for Int levels)"""
    J = np.asarray(J, np.int64)
    assert np.isin(J, np.asarray(levels, np.int64)).all()
    return energy_sparse_int(A, J, sg)


def energy_sparse_f64(A, J, sg):
    """GraphRRGNormal / GraphEANormal (RRG.jl:532-559, EA.jl:584-611): Float64"""
    return _sparse(A, np.asarray(J, np.float64), sg.astype(np.float64))


def energy_skn(J, sg):
    """GraphSKNormal (SK.jl:212-237): -(1/2) Σ_i Σ_j σ_i σ_j J_ij (the diagonal of J is zero)"""
    J = np.asarray(J, np.float64)
    s = sg.astype(np.float64)
    return -0.5 * np.einsum("si,ij,sj->s", s, J, s)


def sk_binary_couplings(Jbits, N):
    """the N x N matrix of ±1 (zero diagonal) of a GraphSK's BitVector rows (SK.jl:28-49: bit j of row i set means J_ij = +1/√N)"""
    Jbits = np.ascontiguousarray(Jbits, np.uint64).reshape(N, -1)
    j = np.arange(N)
    Jpm = 2 * ((Jbits[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int64) - 1
    Jpm[j, j] = 0
    return Jpm


def energy_sk_binary(Jbits, N, sg):
    """GraphSK (SK.jl:62-94; the commented `altn` of :82-91 is the definition): -(1/2) Σ_{i≠j} (2 J_ij − 1) σ_i σ_j / √N"""
    Jpm = sk_binary_couplings(Jbits, N)
    n = -np.einsum("si,ij,sj->s", sg, Jpm, sg)
    assert (n % 2 == 0).all()                                              # SK.jl:77
    return (n // 2) / math.sqrt(N)                                       # SK.jl:93: n / sN


def energy_discretized(A, dJ, rJ, lev_mul, lev_div, sg):
    """GraphRRGNormalDiscretized (RRG.jl:326-355): E0 of the inner level graph (couplings dJ, in level units of lev_mul / lev_div) plus E1 of the
    Float64 residuals rJ"""
    E0 = energy_sparse_int(A, np.asarray(dJ, np.int64), sg) * lev_mul / lev_div
    return E0 + energy_sparse_f64(A, rJ, sg)


def quant_fourK(beta, Gamma, M):
    """QT.jl:165"""
    return round(2.0 / beta * math.log(1.0 / math.tanh(beta * Gamma / M)), 8)


def energy_quant(slice_energy, Nk, M, Gamma, beta, sg):
    """GraphQuant (QT.jl:185-199): energy(X0, C) + Σ_k energy(X1[k], slice k) / M, slice k = spins k Nk .. (k + 1) Nk − 1 (:194), with
    energy(X0) = energy0 · fourK / 4 (QT.jl:84), energy0 = −Σ_i Σ_k σ_(i,k) σ_(i,k−1) around the Trotter ring (QT.jl:68-82)."""
    s = sg.reshape(-1, M, Nk)
    n0 = -(s * np.roll(s, 1, axis=1)).sum(axis=(1, 2))
    E = n0 * quant_fourK(beta, Gamma, M) / 4
    for k in range(M):
        E = E + slice_energy(s[:, k, :]) / M
    return E


def energy_re(slice_energy, Nk, M, gamma, beta, sg):
    """GraphRobustEnsemble (RE.jl:265-281): energy(X0, C) + Σ_k energy(X1[k], replica k), site j = spin j // M of replica j % M (:274), with
    GraphRE's energy(X0) = −Σ_i log(2 cosh(γ μ_i)) / β, μ_i = Σ_k σ_(i,k) (RE.jl:70-88)."""
    s = sg.reshape(-1, Nk, M)
    E = -(np.log(2 * np.cosh(gamma * s.sum(axis=2))) / beta).sum(axis=1)
    if slice_energy is not None:                                           # GraphEmpty: 0 (Empty.jl:28)
        for k in range(M):
            E = E + slice_energy(s[:, :, k])
    return E


def energies(X, sg):
    """E of every state in `sg` ([S, N] of ±1) for a graph object of the product package, by its class name — public arrays only"""
    name = type(X).__name__
    if name in ("GraphRRG", "GraphEA"):
        return energy_sparse_int(X.A, X.J, sg)
    if name in ("GraphRRGLevels", "GraphEALevels"):
        assert X.lev_mul == 1 and X.lev_div == 1.0, "Int levels only"
        return energy_sparse_levels(X.A, X.J, X.levels, sg)
    if name in ("GraphRRGNormal", "GraphEANormal"):
        return energy_sparse_f64(X.A, X.J, sg)
    if name == "GraphSKNormal":
        return energy_skn(X.J, sg)
    if name == "GraphSK":
        return energy_sk_binary(X.J, X.N, sg)
    if name == "GraphRRGNormalDiscretized":
        return energy_discretized(X.A, X.dJ, X.rJ, X.lev_mul, X.lev_div, sg)
    if name == "GraphQuant":
        return energy_quant(lambda s: np.asarray(energies(X.X1, s), np.float64), X.Nk, X.M, X.Gamma, X.beta, sg)
    if name == "GraphRobustEnsemble":
        return energy_re(None if X.X1 is None else (lambda s: np.asarray(energies(X.X1, s), np.float64)), X.Nk, X.M, X.gamma, X.beta, sg)
    raise NotImplementedError(name)


# ---- the statistic ------------------------------------------------------------------------------------------------------------------
def _wilson_hilferty_limit(k):
    # the χ² quantile of the 1e-6 upper tail, Wilson-Hilferty (z = 4.7534 is the normal 1e-6 quantile)
    return k * (1 - 2 / (9 * k) + 4.753424 * (2 / (9 * k)) ** 0.5) ** 3


def boltzmann(E, beta):
    w = -beta * np.asarray(E, np.float64)
    p = np.exp(w - w.max())
    return p / p.sum()


Score = namedtuple("Score", "chi2 limit dof min_expected pooled_expected pooled_mass")


def score(counts, p):
    """Pearson χ² of `counts` against R p.  Bins whose expected count is below 5 are pooled into one, and the degrees of freedom shrink with
    them; `pooled_expected` is that bin's own expected count (inf when nothing was pooled), `pooled_mass` its probability."""
    counts = np.asarray(counts, np.float64)
    R = counts.sum()
    e = R * np.asarray(p, np.float64)
    small = e < 5
    if small.any():
        c, ee = np.append(counts[~small], counts[small].sum()), np.append(e[~small], e[small].sum())
    else:
        c, ee = counts, e
    dof = len(ee) - 1
    return Score(float(((c - ee) ** 2 / ee).sum()), _wilson_hilferty_limit(dof), dof, float(e.min()),
                 float(e[small].sum()) if small.any() else math.inf, float(np.asarray(p)[small].sum()))


def check_pooling(sc):
    assert sc.dof >= 1
    assert sc.pooled_expected >= 5, "the pooled bin's own expected count is %.2f" % sc.pooled_expected
    assert sc.pooled_mass <= 0.05, "the pooled bins hold %.3f of the mass" % sc.pooled_mass


def energy_levels(E, tol=1e-9):
    """(levels, level_of_state): the distinct energies of the enumerated states (values closer than `tol` are one level — for Gaussian couplings
    a level is one state and its global flip)"""
    E = np.asarray(E, np.float64)
    order = np.argsort(E, kind="stable")
    new = np.concatenate([[True], np.diff(E[order]) > tol])
    lev_sorted = np.cumsum(new) - 1
    level_of_state = np.empty(len(E), np.int64)
    level_of_state[order] = lev_sorted
    levels = np.array([E[order][lev_sorted == k].mean() for k in range(lev_sorted[-1] + 1)])
    return levels, level_of_state


def level_index(levels, Es):
    """the level each sampled energy belongs to; asserts that it is one (|E − level| <= 1e-9 max(1, |E|))"""
    Es = np.asarray(Es, np.float64)
    k = np.clip(np.searchsorted((levels[1:] + levels[:-1]) / 2, Es), 0, len(levels) - 1)
    assert (np.abs(Es - levels[k]) <= 1e-9 * np.maximum(1.0, np.abs(Es))).all(), "a sampled energy is no energy of any state"
    return k


Verdict = namedtuple("Verdict", "law power")          # two Scores: against the law at β, and against the law at power·β


def judge(case, E, idx, Es_last, power=1.1):
    """The counts of a run against the law at case.beta and at power·case.beta.  observable "state": the final configurations `idx`, one bin per
    state; "energy": the last sampled energies `Es_last`, one bin per exact energy level."""
    if case.observable == "state":
        counts = np.bincount(idx, minlength=len(E))
        p, q = boltzmann(E, case.beta), boltzmann(E, power * case.beta)
    else:
        levels, lev = energy_levels(E)
        counts = np.bincount(level_index(levels, Es_last), minlength=len(levels))
        p = np.bincount(lev, weights=boltzmann(E, case.beta), minlength=len(levels))
        q = np.bincount(lev, weights=boltzmann(E, power * case.beta), minlength=len(levels))
    return Verdict(score(counts, p), score(counts, q))


def assert_verdict(v):
    check_pooling(v.law)
    check_pooling(v.power)
    assert v.law.chi2 < v.law.limit, "χ² %.1f against the Boltzmann law exceeds the 1e-6 limit %.1f (%d dof)" % (v.law.chi2, v.law.limit, v.law.dof)
    assert v.power.chi2 > v.power.limit, ("no power: the same counts pass the law at the wrong β too (χ² %.1f, limit %.1f)"
                                          % (v.power.chi2, v.power.limit))


def assert_tracked_energy(E, idx, Etr):
    """the energy a chain tracked equals the definition's energy of its final state: exactly for integers, to 1e-12 max(1, |E|) for Float64"""
    Eref = np.asarray(E)[idx]
    if np.issubdtype(np.asarray(E).dtype, np.integer):
        assert np.issubdtype(np.asarray(Etr).dtype, np.integer) and (np.asarray(Etr) == Eref).all()
    else:
        assert (np.abs(np.asarray(Etr, np.float64) - Eref) <= 1e-12 * np.maximum(1.0, np.abs(Eref))).all(), float(np.abs(Etr - Eref).max())


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# model: a function of the package that builds the graph, with explicit tiny parameters.  sampler: std | fast | colored | rrr | bkl | wtm.
# iters: iterations (std, fast, rrr, bkl), sweeps (colored) or global time in units of 1/N (wtm, taken as 4 samples).  env: the switches that
# select a kernel build (existing ones; the table adds none).  observable: what is binned —
#   "state":  the configuration the call leaves behind.  standardMC, rrrMC, the fast mode and the colour sweeps make exactly `iters` moves
#             (src/RRRMC.jl:100-119, 180-209, 249-281): that configuration is the chain's state at a fixed iteration count.
#   "energy": the last sampled energy Es[:, -1], over the exact energy levels.  bklMC and wtmMC sample at fixed iteration counts / times but
#             leave the loop from inside the sampling `while` (src/RRRMC.jl:339-344, 402-407) — the law is stated for the samples, so the rows
#             use those (that the configuration left behind is the sampled one is asserted as well, through its tracked energy).
# cpu_R: chains of the CPU twin (the oracle; None: no oracle entry point).  cpu_power: the wrong-β factor the reduced run must tell apart.
Case = namedtuple("Case", "id model sampler beta R iters seed env observable cpu_R cpu_power staged_thr")


def _case(id, model, sampler, beta, iters, seed, R=65536, env=None, observable=None, cpu_R=8192, cpu_power=1.1, staged_thr=None):
    if observable is None:
        observable = "energy" if sampler in ("bkl", "wtm") else "state"
    return Case(id, model, sampler, beta, R, iters, seed, dict(env or {}), observable, cpu_R, cpu_power, staged_thr)


def _rrg(N, K, seed):
    return lambda pkg: pkg.GraphRRG(N, K, seed=seed)


def _rrgn(N, K, seed):
    return lambda pkg: pkg.GraphRRGNormal(N, K, seed=seed)


def _quant_rrg(pkg):
    return pkg.GraphQuant(pkg.GraphRRG(3, 2, seed=31), 3, 0.8, 0.9)             # GraphQuant over the triangle: Nk M = 9, 512 states


def _qskt(pkg):
    return pkg.GraphQSKT(3, 3, 0.8, 0.9, seed=32)                              # binary SK slices, Nk M = 9


def _qeat(pkg):
    return pkg.GraphQEAT(3, 1, 3, 0.8, 0.9, seed=33)                           # Float64 slices on the 3-ring (L = 3, D = 1), Nk M = 9


def _dbl(pkg):
    return pkg.GraphRRGNormalDiscretized(8, 3, (-1, 0, 1), seed=21)


def _colored_ea(pkg):
    X = pkg.GraphEA(2, 3, seed=7)
    X.coloring = pkg.checkerboard_coloring(2, 3)
    return X


def _colored_rrg(pkg):
    import oracle
    X = pkg.GraphRRG(8, 3, seed=8)
    X.coloring = oracle.greedy_coloring(X.A)
    return X


PM1 = _rrg(8, 3, 11)                  # the ±J graph of most rows: 256 states, energies in steps of 2
CASES = [
    # -- chains that are not the reference's
    _case("fast-RRGNormal-K3-spf_fast_kernels", _rrgn(8, 3, 5), "fast", 0.7, 2400, 101),
    _case("fast-RRGNormal-K4-spf_fast_kernels", _rrgn(8, 4, 6), "fast", 0.5, 2400, 102),
    _case("fast-RRGNormal-K3-negative-beta-spf_fast_kernels", _rrgn(8, 3, 5), "fast", -0.7, 2400, 103),
    _case("colored-EA-checkerboard-colored_sweep_kernel", _colored_ea, "colored", 0.25, 300, 104),
    _case("colored-RRG-greedy-colored_sweep_kernel", _colored_rrg, "colored", 0.6, 300, 105),
    # -- standardMC
    _case("std-RRG-sweep_kernel", PM1, "std", 0.6, 2400, 111),
    _case("std-RRG-levels-lev_kernel", lambda pkg: pkg.GraphRRG(8, 3, (-1, 0, 1), seed=12), "std", 0.8, 2400, 112),
    _case("std-RRGNormal-spf_team_kernel", _rrgn(8, 3, 5), "std", 0.7, 2400, 113),
    _case("std-RRGNormal-spf_sweep_kernel", _rrgn(8, 3, 5), "std", 0.7, 2400, 114, env={"RRRMC_SPF_TEAM": "0"}),
    _case("std-SKNormal-sk_block_kernel", lambda pkg: pkg.GraphSKNormal(8, seed=13), "std", 1.0, 2400, 115),
    _case("std-SK-binary-sk_kernels", lambda pkg: pkg.GraphSK(8, seed=14), "std", 0.9, 2400, 116, cpu_power=1.2),
    _case("std-RRGNormalDiscretized-dbl_kernels", _dbl, "std", 0.7, 2400, 117),
    _case("std-Quant-RRG-quant_kernels", _quant_rrg, "std", 0.9, 2700, 118, cpu_R=16384),
    _case("std-QSKT-quant_kernels", _qskt, "std", 0.9, 2700, 119),
    _case("std-QEAT-quant_kernels", _qeat, "std", 0.9, 2700, 120),
    _case("std-Graph0RE-re_kernels", lambda pkg: pkg.Graph0RE(3, 3, 0.6, 1.2), "std", 1.0, 2700, 121, cpu_R=None),
    _case("std-GraphSKRE-re_kernels", lambda pkg: pkg.GraphSKRE(3, 3, 0.6, 1.2, seed=15), "std", 0.8, 2700, 122, cpu_R=None),
    _case("std-RRG-big_kernels", PM1, "std", 0.6, 2400, 123, env={"RRRMC_FORCE_BIG": "1"}),
    _case("std-RRG-sweep_kernel-wide", PM1, "std", 0.6, 2400, 124, env={"RRRMC_FORCE_WIDE": "1"}),
    _case("std-RRG-sweep_kernel-single", PM1, "std", 0.6, 2400, 125, env={"RRRMC_FORCE_SINGLE": "1"}),
    # -- rrrMC.  The LDS/wave build runs one workgroup per replica and is chosen for few replicas only: RRRMC_RRR_WAVE_MAX_R lifts that bound.
    # cont_wave_kernel (GraphRRGNormal) refuses N < 64 (host_spf.hpp), which cannot be enumerated: it has no row; the thread build, which
    # RRRMC_CONT_NO_WAVE=1 selects at any N, is what runs here.
    _case("rrr-RRG-sparse_wave_kernel", PM1, "rrr", 0.6, 1200, 131, env={"RRRMC_RRR_WAVE_MAX_R": "1000000"}),
    _case("rrr-RRG-rrr_sparse_kernel", PM1, "rrr", 0.6, 1200, 132, env={"RRRMC_RRR_NO_WAVE": "1"}),
    _case("rrr-RRGNormal-cont_sparse_kernel", _rrgn(8, 3, 5), "rrr", 0.7, 1200, 133, env={"RRRMC_CONT_NO_WAVE": "1"}),
    _case("rrr-SKNormal-DynamicSampler", lambda pkg: pkg.GraphSKNormal(8, seed=13), "rrr", 1.0, 1200, 134),
    _case("rrr-SK-binary", lambda pkg: pkg.GraphSK(8, seed=14), "rrr", 0.9, 1200, 135, cpu_power=1.2),
    _case("rrr-RRGNormalDiscretized-staged0", _dbl, "rrr", 0.7, 1200, 136, staged_thr=0.0),
    _case("rrr-RRGNormalDiscretized-staged1", _dbl, "rrr", 0.7, 1200, 137, staged_thr=1.0),
    _case("rrr-Quant-RRG", _quant_rrg, "rrr", 0.9, 1350, 138, cpu_R=16384),
    _case("rrr-QSKT", _qskt, "rrr", 0.9, 1350, 139),
    _case("rrr-QEAT", _qeat, "rrr", 0.9, 1350, 140),
    _case("rrr-GraphSKRE-re_kernels", lambda pkg: pkg.GraphSKRE(3, 3, 0.6, 1.2, seed=15), "rrr", 0.8, 1350, 141, cpu_R=None),
    # -- bklMC and wtmMC: the last sampled energy over the energy levels
    _case("bkl-RRG", PM1, "bkl", 0.3, 2400, 151, cpu_R=16384),
    _case("bkl-RRGNormal", _rrgn(8, 3, 5), "bkl", 0.7, 2400, 152),
    _case("bkl-SKNormal", lambda pkg: pkg.GraphSKNormal(8, seed=13), "bkl", 1.0, 2400, 153),
    _case("wtm-RRG", PM1, "wtm", 0.3, 2400, 161, cpu_R=16384),
    _case("wtm-RRGNormal", _rrgn(8, 3, 5), "wtm", 0.7, 2400, 162),
    _case("wtm-SKNormal", lambda pkg: pkg.GraphSKNormal(8, seed=13), "wtm", 1.0, 2400, 163),
]
CASE_IDS = [c.id for c in CASES]


class with_env:
    """the case's switches for the duration of a block (they are read when a context is made and when a sampler is launched)"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def exact_energies(X):
    return np.asarray(energies(X, 2 * enumerate_states(X.N) - 1))


# ---- the two runners: (final state index[R], tracked energy[R], last sampled energy[R]) ------------------------------------------------
WTM_SAMPLES = 4


def run_engine(pkg, case, X, R=None):
    R = case.R if R is None else R
    with with_env(case.env), pkg.Engine(X, R) as eng:
        eng.seed(case.seed)
        eng.init_spins_random()
        it = case.iters
        if case.sampler == "std":
            Es = eng.standard_mc(case.beta, it, it)[0]
        elif case.sampler == "fast":
            Es = eng.standard_mc_fast(case.beta, it, it)[0]
        elif case.sampler == "colored":
            eng.set_coloring(X.coloring)
            Es = eng.colored_sweeps(case.beta, it, it)
        elif case.sampler == "rrr":
            Es = eng.rrr_mc(case.beta, it, it, staged_thr=case.staged_thr)[0]
        elif case.sampler == "bkl":
            Es = eng.bkl_mc(case.beta, it, it // 4)[0]
        else:
            Es = eng.wtm_mc(case.beta, WTM_SAMPLES, it / WTM_SAMPLES)[0]
        assert Es.shape[0] == R and Es.shape[1] >= 1
        # the fast mode tracks no energy (it evaluates the spins at every sample): its rows hold the library's energy() of the final
        # configuration to the definition instead
        Etr = eng.energy() if case.sampler == "fast" else eng.run_energy()
        return _state_index(eng.get_config(), X.N), Etr, Es[:, -1].copy()


def _oracle_chain(O, case, X):
    """a function (initial chunks, replica) -> (last sampled energy, final chunks) through the oracle's entry point for the case"""
    name, s, beta, it, seed = type(X).__name__, case.sampler, case.beta, case.iters, case.seed
    wstep = it / WTM_SAMPLES
    pick = lambda out: (out[0][-1], out[1])
    if name in ("GraphRRG", "GraphEA"):
        A, J, form = X.A, X.J.astype(np.int32), "ea" if name == "GraphEA" else "rrg"
        if s == "std":
            return lambda ch, r: pick(O.standard_mc_sparse(A, J, beta, it, it, seed, ch, replica=r, form=form))
        if s == "colored":
            return lambda ch, r: pick(O.colored_sweeps_sparse(A, J, X.coloring, beta, it, it, seed, ch, replica=r))
        if s in ("rrr", "bkl"):
            return lambda ch, r: pick(O.rrr_sparse(A, J, beta, it, it if s == "rrr" else it // 4, seed, ch, replica=r, form=form, bkl=s == "bkl"))
        return lambda ch, r: pick(O.wtm_mc_sparse(A, J, beta, WTM_SAMPLES, wstep, seed, ch, replica=r, form=form))
    if name == "GraphRRGLevels" and s == "std":
        return lambda ch, r: pick(O.standard_mc_lev(X.A, X.J.astype(np.int32), beta, it, it, seed, ch, replica=r, mul=X.lev_mul, div=X.lev_div))
    if name == "GraphRRGNormal":
        if s == "std":
            return lambda ch, r: pick(O.standard_mc_spf(X.A, X.J, beta, it, it, seed, ch, replica=r))
        if s == "fast":
            return lambda ch, r: pick(O.standard_mc_spf_fast(X.A, X.J, beta, it, it, seed, ch, replica=r))
        if s == "wtm":
            return lambda ch, r: pick(O.cont_sparse("wtm", X.A, X.J, beta, WTM_SAMPLES, 1, seed, ch, replica=r, stepf=wstep))
        return lambda ch, r: pick(O.cont_sparse(s, X.A, X.J, beta, it, it if s == "rrr" else it // 4, seed, ch, replica=r))
    if name == "GraphSKNormal":
        fn = {"std": lambda ch, r: O.standard_mc_skn(X.J, beta, it, it, seed, ch, replica=r),
              "rrr": lambda ch, r: O.rrr_mc_skn(X.J, beta, it, it, seed, ch, replica=r),
              "bkl": lambda ch, r: O.bkl_mc_skn(X.J, beta, it, it // 4, seed, ch, replica=r),
              "wtm": lambda ch, r: O.wtm_mc_skn(X.J, beta, WTM_SAMPLES, wstep, seed, ch, replica=r)}[s]
        return lambda ch, r: pick(fn(ch, r))
    if name == "GraphSK":
        fn = {"std": lambda ch, r: O.standard_mc_skb(X.J, beta, it, it, seed, ch, replica=r),
              "rrr": lambda ch, r: O.rrr_mc_skb(X.J, beta, it, it, seed, ch, replica=r)}[s]
        return lambda ch, r: pick(fn(ch, r))
    if name == "GraphRRGNormalDiscretized":
        if s == "std":
            return lambda ch, r: pick(O.standard_mc_dbl(X.A, X.dJ, X.rJ, beta, it, it, seed, ch, replica=r, mul=X.lev_mul, div=X.lev_div))
        return lambda ch, r: pick(O.rrr_double_sparse(X.A, X.dJ, X.rJ, X.LEV, beta, it, it, seed, ch, replica=r, staged_thr=case.staged_thr,
                                                      mul=X.lev_mul, div=X.lev_div))
    if name == "GraphQuant":
        M, fK = X.M, X.fourK
        if X.sk_slices:
            f = O.standard_mc_quant_sk if s == "std" else O.rrr_mc_quant_sk
            return lambda ch, r: pick(f(X.J, X.Nk, M, fK, beta, it, it, seed, ch, replica=r))
        if X.f64_slices:
            f = O.standard_mc_quant_spf if s == "std" else O.rrr_mc_quant_spf
            return lambda ch, r: pick(f(X.A, X.J, M, fK, beta, it, it, seed, ch, replica=r))
        f = O.standard_mc_quant if s == "std" else O.rrr_mc_quant
        J = X.J.astype(np.int32)
        return lambda ch, r: pick(f(X.A, J, M, fK, beta, it, it, seed, ch, replica=r))
    raise NotImplementedError("%s under %s has no oracle entry point" % (name, s))


def run_oracle(O, case, X, R, r0=0):
    """chains r0 .. r0 + R − 1 of the case through the oracle, from the INIT stream's configurations (what Engine.init_spins_random draws).
    The tracked energy of an oracle chain at its end is not exported: the last sample stands in for it where the sampler stops at the sample
    (bklMC, wtmMC) and nothing does otherwise (None)."""
    chain = _oracle_chain(O, case, X)
    chunks = np.zeros((R, 1), np.uint64)
    Es = np.zeros(R, np.float64 if X.energy_dtype == np.float64 else np.int64)
    for i in range(R):
        e, ch = chain(O.init_config(case.seed, r0 + i, X.N), r0 + i)
        Es[i], chunks[i] = e, ch
    if type(X).__name__ == "GraphRRGLevels":
        Es = X.energy_value(Es)
    idx = state_index_of_chunks(chunks, X.N)
    return idx, (Es if case.observable == "energy" else None), Es
