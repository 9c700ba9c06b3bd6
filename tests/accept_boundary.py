"""Boundary probes for the accept decision ``x >= 0 || rand() < exp(x)`` (src/RRRMC.jl:39), made with the oracle alone: no GPU, no fixtures.

A random run essentially never puts a move where its verdict depends on the last bits of det_exp, so the kernels that replace
``u < det_exp(x)`` by a filter (sk_block_kernel, sk_hblock_kernel, spf_team_kernel) never take their in-band branch under test.  A probe
is a pair of ADJACENT doubles beta_acc < beta_rej such that attempt ``t`` of replica ``r`` (a move with dE > 0, uniform u) is accepted at
beta_acc and rejected at beta_rej while the chain before it is the same: u sits between det_exp(-beta_acc dE) and det_exp(-beta_rej dE),
two values one or two ulps apart.

The oracle numbers iterations from 1: site_of(seed, g, N) and rand53(seed, g, r) take g = it0 + t.
"""
import math
from collections import namedtuple

import numpy as np

Probe = namedtuple("Probe", "seed r t site u dE beta_acc beta_rej prefix")

CLASSES = (1, 2, 33, 64, 65, 128)          # lane 0, lane 1, lane 32, last lane of block 0, lane 0 of block 1, last lane of block 1
LARGE_X = (-90.0, -110.0, -699.0, -701.0, -722.6, -745.1, -745.3)      # spf_team's |xx| >= 87; both sides of x = -700; subnormal result; both sides of -745.2
LARGE_BETA = (1e5, 1e300, math.inf)


def find_pair(O, run, N, seed, r, t, dE_of=None, delta=None, beta0=1.0, iters=None):
    """``run(beta, iters) -> (accepted, fields_or_None)`` is one oracle chain of replica ``r`` under ``seed`` from its start configuration.
    ``dE_of(fields, site)`` turns the cached field of the attempted site into the move's dE (default: the field itself); a model without a
    field cache passes ``delta(beta, t) -> dE`` instead.  ``iters``: the length of the run the probe is for — its accepted counts at the two
    betas must differ (what a caller can see).  Returns a Probe or None (dE <= 0, or beta moved the prefix)."""
    site, u = O.site_of(seed, t, N), O.rand53(seed, t, r)
    if not 0.0 < u < 1.0:
        return None

    def dE_at(beta):
        if delta is not None:
            return float(delta(beta, t))
        f = run(beta, t - 1)[1]
        return float(f[site] if dE_of is None else dE_of(f, site))

    beta, dE = float(beta0), None
    for _ in range(30):                                   # beta <- -ln(u) / dE(beta) to a fixed point: the prefix depends on beta too
        dE = dE_at(beta)
        if not dE > 0.0:
            return None
        nb = -math.log(u) / dE
        if nb == beta:
            break
        beta = nb
    else:
        return None

    prefix = run(beta, t - 1)[0]

    def state(b):
        """+1 accepted, 0 rejected, None: the chain before attempt t is not the one the pair is made for"""
        p = run(b, t - 1)[0]
        if p != prefix or dE_at(b) != dE:
            return None
        return run(b, t)[0] - p

    lo, hi = beta * (1.0 - 1e-9), beta * (1.0 + 1e-9)
    if state(lo) != 1 or state(hi) != 0:
        return None
    while np.nextafter(lo, math.inf) < hi:
        mid = lo + (hi - lo) / 2.0
        s = state(mid)
        if s is None:
            return None
        if s:
            lo = mid
        else:
            hi = mid
    if iters is not None and run(lo, iters)[0] == run(hi, iters)[0]:
        return None                                       # the two chains part at attempt t; their accepted counts met again by the end of the run
    return Probe(seed, r, t, site, u, dE, float(lo), float(hi), int(prefix))


def find_targets(O, make_run, N, t, R, want=3, seeds=range(1, 65), **kw):
    """The first ``want`` live probes of attempt class ``t`` in the fixed order seed = 1..64, r = 0..R-1, at most one per seed (a GPU run
    takes one seed and one beta for all its replicas).  ``make_run(seed, r)`` returns the keyword arguments of find_pair that depend on the
    chain: ``run`` and, where needed, ``delta``."""
    out = []
    for seed in seeds:
        for r in range(R):
            p = find_pair(O, N=N, seed=seed, r=r, t=t, **make_run(seed, r), **kw)
            if p is not None:
                out.append(p)
                break
        if len(out) >= want:
            break
    return out


def four_betas(p):
    """beta_acc, beta_rej and one further nextafter on each side"""
    return (float(np.nextafter(p.beta_acc, -math.inf)), p.beta_acc, p.beta_rej, float(np.nextafter(p.beta_rej, math.inf)))


def large_x_betas(O, run, N, seed, dE_of=None):
    """For the start configuration behind ``run``: the lane with the largest positive start dE among the 64 attempts of the first block, and
    for each value of LARGE_X the beta that puts x = -beta dE of that lane there WHEN ITS TURN COMES (the accepted moves before it shift its
    field, so beta is iterated to a fixed point), then LARGE_BETA.  Returns (lane, site, [(x_target or None, beta, x_actual), ...]); x_actual
    is computed from the oracle's fields after ``lane`` attempts at that beta."""
    dE = (lambda f, s: float(f[s])) if dE_of is None else dE_of
    f0 = run(1.0, 0)[1]
    cand = [(dE(f0, O.site_of(seed, l + 1, N)), l) for l in range(64)]
    d0, lane = max(cand)
    if not d0 > 0.0:
        return None
    site = O.site_of(seed, lane + 1, N)
    out = []
    for x in LARGE_X:
        beta = -x / d0
        for _ in range(30):
            d = dE(run(beta, lane)[1], site)
            if not d > 0.0:
                return None
            nb = -x / d
            if nb == beta:
                break
            beta = nb
        else:
            return None                                   # (beta keeps moving the prefix: the caller takes another seed)
        out.append((x, beta, -beta * dE(run(beta, lane)[1], site)))
    for beta in LARGE_BETA:
        out.append((None, beta, -beta * dE(run(beta, lane)[1], site)))
    return lane, site, out


def ulp(v):
    """spacing of the doubles at |v| (the subnormal grid below 2^-1022)"""
    return float(np.spacing(abs(float(v))))


# ---- the oracle's side of the paths the probes run on ---------------------------------------------------------------------------------
class Path:
    """One model on the oracle: ``make_run(seed, r)`` for find_targets, ``ref(seed, beta, iters, R)`` = what a device run of R replicas
    from init_spins_random must return at step = 1: (Es[R, iters], configs[R], accepted[R], fields[R] or None)."""

    def __init__(self, O, N, chain, dE_of=None, energy=None):
        self.O, self.N, self.chain, self.dE_of, self.energy = O, N, chain, dE_of, energy

    def make_run(self, seed, r):
        c0 = self.O.init_config(seed, r, self.N)

        def run(beta, iters):
            o = self.chain(beta, iters, seed, c0, r)
            return o[2], (o[3] if len(o) > 3 else None)

        kw = {"run": run}
        if self.dE_of is not None:
            kw["dE_of"] = self.dE_of
        if self.energy is not None:                     # no field cache: dE of attempt t from the definition, E(flipped) - E

            def delta(beta, t):
                c = self.chain(beta, t - 1, seed, c0, r)[1].copy()
                i = self.O.site_of(seed, t, self.N)
                E0 = self.energy(c)
                c[i >> 6] ^= np.uint64(1) << np.uint64(i & 63)
                return self.energy(c) - E0

            kw["delta"] = delta
        return kw

    def ref(self, seed, beta, iters, R):
        outs = [self.chain(beta, iters, seed, self.O.init_config(seed, r, self.N), r) for r in range(R)]
        lf = np.stack([o[3] for o in outs]) if len(outs[0]) > 3 else None
        return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.array([o[2] for o in outs], np.int64), lf


def sk_path(O, N, binary, gseed):
    """GraphSKNormal (dE = lfields[i], SK.jl:278-284) / binary GraphSK (dE = lfields[i] / sqrt(N), SK.jl:137-140)"""
    J = O.gen_sk_binary(N, gseed) if binary else O.gen_sk_gauss(N, gseed)
    fn = O.standard_mc_skb if binary else O.standard_mc_skn
    sN = math.sqrt(N)
    p = Path(O, N, lambda beta, iters, seed, c0, r: fn(J, beta, iters, 1, seed, c0, replica=r),
             dE_of=(lambda f, s: float(f[s]) / sN) if binary else None)
    p.J = J
    return p


def spf_path(O, kind, a, b, gseed):
    """GraphRRGNormal(N = a, K = b) / GraphEANormal(L = a, D = b): dE = -lfields[i] (RRG.jl:619-625)"""
    A = O.gen_rrg(a, b, gseed) if kind == "rrg" else O.gen_ea(a, b)
    J = O.gen_couplings_gauss(A, gseed)
    p = Path(O, A.shape[0], lambda beta, iters, seed, c0, r: O.standard_mc_spf(A, J, beta, iters, 1, seed, c0, replica=r, form=kind),
             dE_of=lambda f, s: -float(f[s]))
    p.A, p.J = A, J
    return p


def qeat_path(O, L, D, M, Gamma, beta_g, gseed):
    """GraphQEAT = GraphQuant over GraphEANormal slices (QAliases.jl:50-83): no field accessor, dE from the energy's definition"""
    A = O.gen_ea(L, D)
    J = O.gen_couplings_gauss(A, gseed)
    fourK = O.quant_fourK(beta_g, Gamma, M)
    p = Path(O, A.shape[0] * M, lambda beta, iters, seed, c0, r: O.standard_mc_quant_spf(A, J, M, fourK, beta, iters, 1, seed, c0, replica=r),
             energy=lambda c: O.quant_spf_energy(A, J, M, fourK, c))
    p.A, p.J, p.fourK = A, J, fourK
    return p


# ---- the paths of the suite: the CPU tests check every target, the GPU tests run them -------------------------------------------------
GSEED = 4242                               # the graphs' seed (the runs' seeds are the targets')
SK_SIZES = (37, 300, 1100)                 # one site per thread of 256; 512 threads with a partial tile; three sites per thread
R_SK, R_SPF, R_CTL = 9, 70, 5              # a padded group of 8; a partial last team of 64 / 32 / 16; the control
QEAT = (4, 2, 8, 0.5, 2.0)                 # L, D, M, Gamma, beta of the control graph (N = 128)
PATHS = {("skn", N): R_SK for N in SK_SIZES}
PATHS.update({("skb", N): R_SK for N in SK_SIZES})
PATHS.update({("rrgn", 96): R_SPF, ("ean", 16): R_SPF, ("qeat", 128): R_CTL})
_paths, _targets = {}, {}


def path(O, key):
    """("skn" | "skb", N): dense SK; ("rrgn", 96): GraphRRGNormal(96, 3); ("ean", 16): GraphEANormal(2, 4), K = 8; ("qeat", 128): the control"""
    if key not in _paths:
        kind, N = key
        _paths[key] = (sk_path(O, N, kind == "skb", GSEED + N) if kind in ("skn", "skb") else spf_path(O, "rrg", 96, 3, GSEED) if kind == "rrgn"
                       else spf_path(O, "ea", 2, 4, GSEED) if kind == "ean" else qeat_path(O, *QEAT, GSEED))
    return _paths[key]


def classes_of(key):
    return (1, 2) if key[0] == "qeat" else CLASSES


def targets(O, key, t):
    """the probes of (path, attempt class): computed once per process, the same on every run"""
    if (key, t) not in _targets:
        p = path(O, key)
        _targets[(key, t)] = find_targets(O, p.make_run, p.N, t, PATHS[key], iters=iters_for(t))
    return _targets[(key, t)]


LARGE_X_PATHS = (("skn", 37), ("skn", 300), ("skb", 37), ("skb", 300), ("rrgn", 96), ("ean", 16))
_large = {}


def large_x_case(O, key):
    """(seed, r = 0, lane, site, [(x_target or None, beta, x_actual)]) of the first seed in 1..64 whose start block has a lane for every
    value of LARGE_X"""
    if key not in _large:
        p = path(O, key)
        for seed in range(1, 65):
            kw = p.make_run(seed, 0)
            got = large_x_betas(O, kw["run"], p.N, seed, kw.get("dE_of"))
            if got is not None:
                _large[key] = (seed, 0) + got
                break
    return _large[key]


def iters_for(t):
    return 64 * ((t + 63) // 64) + 64
