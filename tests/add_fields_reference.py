"""Plain-Python restatement of GraphAddFields / GraphAddSubFields (src/graphs/AddFields.jl:16-123) and of rrrMC(X::DoubleGraph)
(src/RRRMC.jl:221-290) over DeltaECacheCont (src/DeltaE.jl:297-410) and the DynamicSampler (src/DynamicSamplers.jl; tests/tape_replay.py)
of the inner graph GraphAF, on the library's addressed random streams.  The wrapped graph g is any object with the slice
interface of re_reference / perc_reference / comm_reference / comm_qu_reference / sat_reference: ``energy(s)`` (which also builds g's
cache), ``delta(s, i)`` and ``flip_update(s, i)`` after the flip of ``s[i]``."""
import numpy as np

import re_reference as RE
import tape_replay as TR

FLOATMIN = 2.2250738585072014e-308


def fdiv(a, b):
    """a / b as IEEE arithmetic gives it (±Inf, NaN where Python raises): z′ of a direct move can be exactly 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


class PrecisionLoss(Exception):
    """DynamicSamplers.jl:147"""


class Sampler(TR.DynamicSampler):
    """tape_replay's DynamicSampler with the branch of getel that a tape must not reach: a draw that lands beyond N or on a weight of
    exactly 0 refreshes once and descends again with the x it was left with (DynamicSamplers.jl:146-150)"""

    getel_refreshes = 0                                     # refreshes made by getel itself (not by setindex!'s counter)

    def getel(self, x):
        while True:
            x *= self.z
            k, off = 0, 1
            for _ in range(self.levs):
                p = self.ps[off + k - 1]
                k *= 2
                if x > p:
                    x -= p
                    k += 1
                off *= 2
            if k >= self.N or self.v[k] == 0:
                if not self.trefresh > 0:
                    raise PrecisionLoss("Unrecoverable loss of precision detected in the dynamic sampler")
                self.refresh()
                self.getel_refreshes += 1
                continue
            return k + 1


class AddFields:
    """GraphAddFields (sub = False) / GraphAddSubFields (sub = True) of the fields h over g"""

    def __init__(self, h, g, sub):
        self.h, self.g, self.sub, self.N = [float(x) for x in h], g, bool(sub), len(h)

    def energy0(self, s):                                   # energy(X0, C), AddFields.jl:33-43
        E = 0.0
        for i in range(self.N):
            E += self.h[i] * (2 * int(s[i]) - 1)
        return E

    def delta0(self, s, i):                                 # delta_energy(X0, C, i) = -2 σ h, AddFields.jl:45-52
        return (-2 * (2 * int(s[i]) - 1)) * self.h[i]

    def energy(self, s):                                    # :81, :117 (g's energy also resets g's cache)
        Eg = float(self.g.energy(s))
        return Eg if self.sub else self.energy0(s) + Eg

    def residual(self, s, i):                               # delta_energy_residual, :83, :119
        dg = float(self.g.delta(s, i))
        return dg - self.delta0(s, i) if self.sub else dg

    def delta(self, s, i):                                  # delta_energy, :85-88, :121
        dg = float(self.g.delta(s, i))
        return dg if self.sub else self.delta0(s, i) + dg

    def spinflip(self, s, i):                               # spinflip!(X, C, i): the bit, then update_cache!(X.X1, C, i)
        s[i] ^= 1
        self.g.flip_update(s, i)


def standard_mc(X, s, beta, iters, step, seed, oracle, replica=0, it0=0, E=None, hook=None):
    """standardMC (RRRMC.jl:81-127).  E = None: a fresh call (E = energy(X, C)); else continue with the given tracked E."""
    if E is None:
        E = X.energy(s)
    Es, accepted = [], 0
    for it in range(1, iters + 1):
        if it % step == 0:
            Es.append(E)
            if hook is not None and not hook(it, s, accepted, E):
                break
        g = it0 + it
        move = oracle.site_of(seed, g, X.N)
        dE = X.delta(s, move)
        x = -beta * dE
        if not (x >= 0 or oracle.rand53(seed, g, replica) < oracle.det_exp(x)):
            continue
        X.spinflip(s, move)
        E += dE
        accepted += 1
    return Es, E, accepted


class AfRun:
    """rrrMC(X::DoubleGraph) on the family as a resumable chain: __init__ is the call's start (energy, gen_ΔEcache(X0, C, β)), run(n) the loop"""

    def __init__(self, X, s, beta, seed, oracle, replica=0, it0=0, staged_thr=0.5, staged_thr_fact=5.0):
        self.X, self.s, self.beta, self.seed, self.O, self.rep = X, s, float(beta), seed, oracle, replica
        self.E = X.energy(s)
        self.dEs = [X.delta0(s, i) for i in range(X.N)]                            # DeltaE.jl:304-313
        self.ds = Sampler([self.prior(self.beta * d) for d in self.dEs])
        self.lam = staged_thr_fact / X.N                                           # RRRMC.jl:243
        self.staged_thr = staged_thr
        self.acc_rate = 0.5
        self.it, self.g0 = 0, it0
        self.accepted = self.staged_its = 0

    def prior(self, x):                                     # DeltaE.jl:297
        return self.O.det_exp(-x) if x > 0 else 1.0

    def _uniform_accept(self, c, x, g):                     # accept(c, x), RRRMC.jl:40-44; the uniform is drawn only where it is read
        if c >= 1 and x >= 0:
            return True
        a = c * self.O.det_exp(x)
        if a >= 1:
            return True
        w = RE.rrr_draws(self.O, self.seed, g, self.rep, 1)
        return RE._u53(w[0], w[1]) < a

    def apply_move(self, move):                             # DeltaE.jl:378-410: X0 has no neighbours, one setindex!
        self.X.spinflip(self.s, move)
        z = self.ds.z
        d = self.X.delta0(self.s, move)
        self.dEs[move] = d
        self.ds.set(move + 1, self.prior(self.beta * d))
        return fdiv(z, self.ds.z)

    def run(self, n, step, hook=None, after=None):
        X, s, ds, N = self.X, self.s, self.ds, self.X.N
        Es = []
        for _ in range(n):
            self.it += 1
            it = self.it
            if it % step == 0:
                Es.append(self.E)
                if hook is not None and not hook(it, s, self.accepted, self.E):
                    break
            g = self.g0 + it
            w = RE.rrr_draws(self.O, self.seed, g, self.rep, 0)
            move = ds.getel(RE._u53(w[0], w[1])) - 1                               # rand_move, DeltaE.jl:326-332
            dE0 = self.dEs[move]
            acc = False
            if self.acc_rate < self.staged_thr:
                self.staged_its += 1
                dEp = -dE0                                                         # compute_staged!: flip, look, flip back
                pp = self.prior(self.beta * dEp)
                zp = ds.z + (pp - ds.v[move])                                      # compute_reverse_probabilities!
                zp = float(N) if zp > N else FLOATMIN if zp < FLOATMIN else zp
                c = fdiv(ds.z, zp)
                dE1 = X.residual(s, move)
                if self._uniform_accept(c, -self.beta * dE1, g):
                    X.spinflip(s, move)
                    self.dEs[move] = dEp                                           # apply_staged!
                    ds.set(move + 1, pp)
                    self.E += dE0 + dE1
                    self.accepted += 1
                    acc = True
            else:
                dE1 = X.residual(s, move)
                c = self.apply_move(move)
                if self._uniform_accept(c, -self.beta * dE1, g):
                    self.E += dE0 + dE1
                    self.accepted += 1
                    acc = True
                else:
                    self.apply_move(move)
            self.acc_rate = self.acc_rate * (1 - self.lam) + (1.0 if acc else 0.0) * self.lam
            if after is not None:
                after(self)
        return Es

    def cache_view(self):
        """what rrrmc_af_cache returns: (ΔEs, v, z, trefresh)"""
        return list(self.dEs), list(self.ds.v[:self.X.N]), self.ds.z, self.ds.trefresh


def slice_of(g):
    """the reference object of a product graph g (None: GraphEmpty needs N, see ``reference_of``), from its public arrays"""
    import comm_qu_reference as CQ
    import comm_reference as CR
    import perc_reference as PR
    import sat_reference as SR
    name = type(g).__name__
    if name == "GraphSK":
        return RE.SliceSK(g.J, g.N)
    if name == "GraphSKNormal":
        return RE.SliceSKN(g.J)
    if name in ("GraphPercStep", "GraphPercLinear"):
        return PR.make(g.patterns(), name == "GraphPercLinear")
    if name in ("GraphCommStep", "GraphCommReLU"):
        return CR.make(g.K2, g.patterns(), g.labels())
    if name == "GraphCommQu":
        return CQ.make(g.K2, g.patterns(), g.labels())
    if name == "GraphSAT":
        return SR.SatRef(g.N, g.A, g.J)
    raise NotImplementedError(name)


def reference_of(X):
    """the restatement of a product GraphAddFields / GraphAddSubFields, with a fresh g"""
    g = RE.SliceEmpty(X.N) if X.X1 is None else slice_of(X.X1)
    return AddFields(X.fields, g, type(X).__name__ == "GraphAddSubFields")
