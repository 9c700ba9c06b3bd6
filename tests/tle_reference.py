"""Plain-Python restatement of the Topological Local Entropy ensemble — TEST INFRASTRUCTURE, written from the Julia sources
(src/graphs/TLE.jl, src/TLEAliases.jl, src/RRRMC.jl:81-127 and :221-290, src/DeltaE.jl:26-295), not from the HIP code.

The generic pieces come from ``re_reference.py`` / ``le_reference.py`` / ``sat_reference.py`` (ArraySet, the slice graphs, findk, the rrrMC
loop, the stream draws).  What is TLE's own is restated literally here: GraphTLE's two integer LocalFields with update_cache!'s move_last
swap (TLE.jl:79-299), neighbors (TLE.jl:313-333), allΔE (TLE.jl:335-347), the constructor's checks (TLE.jl:27-46), the DoubleGraph and the
observables.  Sites are 0-based: site j is spin i = j // (M+1) of the centre when j % (M+1) == 0, of replica j % (M+1) otherwise."""
import numpy as np

import le_reference as LE
import re_reference as RE
import sat_reference as SR
from le_reference import findk
from re_reference import ArraySet, chunks_from_config, config_from_chunks, make_slices  # noqa: F401


def check_neighb(Nk, M, neighb):
    """GraphTLE's constructor checks (TLE.jl:27-46)"""
    if M <= 2:
        raise ValueError("M must be greater than 2, given: %d" % M)
    if len(neighb) != Nk:
        raise ValueError("invalid neighb argument, expected length %d, given: %d" % (Nk, len(neighb)))
    for i, ni in enumerate(neighb):
        if not all(0 <= j < Nk for j in ni):
            raise ValueError("invalid neighb[%d] argument, all elements must be between 1 and %d" % (i + 1, Nk))
        if i in ni:
            raise ValueError("invalid neighb[%d], contains itself" % (i + 1))
        for i1 in range(len(ni)):
            for i2 in range(i1 + 1, len(ni)):
                if ni[i1] == ni[i2]:
                    raise ValueError("duplicated element %d in neighb[%d]" % (i1 + 1, i + 1))
    for i, ni in enumerate(neighb):
        for i1 in ni:
            if i not in neighb[i1]:
                raise ValueError("neighb is not symmetrical, %d ∈ ∂%d but %d ∉ ∂%d" % (i1 + 1, i + 1, i + 1, i1 + 1))


def all_delta_e(M, gT, lT, maxdeg):
    """allΔE(GraphTLE{M,γT,λT}) (TLE.jl:335-347): sort(unique(abs.(ΔE1 .+ ΔE2')))"""
    if M % 2 == 0:
        e1 = [4 * d * gT for d in range(M // 2 + 1)]
        e1.insert(1, 2 * gT)
    else:
        e1 = [2 * (2 * d - 1) * gT for d in range(1, (M + 1) // 2 + 1)]
    mn = M * maxdeg
    e2 = [2 * d * lT for d in range(-mn, mn + 1)]
    return sorted({abs(a + b) for a in e1 for b in e2})


class GraphTLE:
    """the inner graph: two LocalFields{Int} (lfields, lfields_last, move_last; -1 = none)"""

    def __init__(self, Nk, M, gT, lT, neighb):
        check_neighb(Nk, M, neighb)
        self.Nk, self.M, self.gT, self.lT = Nk, M, gT, lT
        self.N = Nk * (M + 1)
        self.neighb = [list(ni) for ni in neighb]
        self.neighb_jcs = [[i1 * (M + 1) for i1 in ni] for ni in neighb]
        self.neighb_Us = [[range(i1 * (M + 1), (i1 + 1) * (M + 1)) for i1 in ni] for ni in neighb]
        self.lf1, self.ll1 = [0] * self.N, [0] * self.N
        self.lf2, self.ll2 = [0] * self.N, [0] * self.N
        self.move_last1 = self.move_last2 = -1
        self.maxdeg = max(len(ni) for ni in neighb)

    def energy(self, s):                     # TLE.jl:79-142
        M, Nk = self.M, self.Nk
        lf1, lf2 = self.lf1, self.lf2
        n = 0
        j = -1
        for i in range(Nk):
            j += 1
            jc = j
            sc = 2 * int(s[jc]) - 1
            mu = 0
            for k in range(1, M + 1):
                j += 1
                sj = 2 * int(s[j]) - 1
                lf1[j] = sc * sj
                mu += sj
            f = sc * mu
            lf1[jc] = f
            n -= f
        self.move_last1 = -1
        self.ll1 = [0] * self.N
        r = 0
        for y in range(self.N):
            lf2[y] = 0
        for i1, ni in enumerate(self.neighb):
            jc1 = i1 * (M + 1)
            sc1 = 2 * int(s[jc1]) - 1
            mu = 0
            for i2 in ni:
                jc2 = i2 * (M + 1)
                sc2 = 2 * int(s[jc2]) - 1
                sc = sc1 * sc2
                for k in range(1, M + 1):
                    j1 = k + i1 * (M + 1)
                    j2 = k + i2 * (M + 1)
                    sj = (2 * int(s[j1]) - 1) * (2 * int(s[j2]) - 1)
                    lf2[j1] += sc * sj
                    lf2[j2] += sc * sj
                    mu += sc2 * sj
            f = sc1 * mu
            lf2[jc1] = 2 * f
            r -= f
        assert r % 2 == 0
        r //= 2
        for y in range(self.N):
            assert lf2[y] % 2 == 0
            lf2[y] //= 2
        self.move_last2 = -1
        self.ll2 = [0] * self.N
        return n * self.gT + r * self.lT

    def update_cache(self, s, move):         # TLE.jl:156-299, after the flip of s[move]
        M = self.M
        k = move % (M + 1)
        i = move // (M + 1)
        jc = i * (M + 1)
        lf1, ll1, lf2, ll2 = self.lf1, self.ll1, self.lf2, self.ll2
        if k != 0:
            jcs = self.neighb_jcs[i]
        else:
            Ux = range(jc, jc + M + 1)
            Us = self.neighb_Us[i]
        assert self.move_last1 == self.move_last2
        if self.move_last1 == move:
            if k != 0:
                lf1[jc], ll1[jc] = ll1[jc], lf1[jc]
                lf1[move], ll1[move] = ll1[move], lf1[move]
            else:
                for y in Ux:
                    lf1[y], ll1[y] = ll1[y], lf1[y]
            if k != 0:
                lf2[jc], ll2[jc] = ll2[jc], lf2[jc]
                lf2[move], ll2[move] = ll2[move], lf2[move]
                for jc1 in jcs:
                    lf2[jc1], ll2[jc1] = ll2[jc1], lf2[jc1]
                    j1 = jc1 + k
                    lf2[j1], ll2[j1] = ll2[j1], lf2[j1]
            else:
                for y in Ux:
                    lf2[y], ll2[y] = ll2[y], lf2[y]
                for u in Us:
                    for y in u:
                        lf2[y], ll2[y] = ll2[y], lf2[y]
            return
        if k != 0:
            sx = 2 * int(s[move]) - 1
            sc = 2 * int(s[jc]) - 1
            lfc = lf1[jc]
            lfm = lf1[move]
            ll1[jc] = lfc
            ll1[move] = lfm
            lf1[jc] = lfc + 2 * (sc * sx)
            lf1[move] = -lfm
        else:
            for y in Ux:
                lfy = lf1[y]
                ll1[y] = lfy
                lf1[y] = -lfy
        self.move_last1 = move
        if k != 0:
            sx = 2 * int(s[move]) - 1
            lfm = lf2[move]
            ll2[move] = lfm
            lf2[move] = -lfm
            sc = 2 * int(s[jc]) - 1
            lfc = lf2[jc]
            ll2[jc] = lfc
            for jc1 in jcs:
                j1 = jc1 + k
                lfj1 = lf2[j1]
                lfc1 = lf2[jc1]
                ll2[j1] = lfj1
                ll2[jc1] = lfc1
                sj1 = 2 * int(s[j1]) - 1
                sc1 = 2 * int(s[jc1]) - 1
                sg = sx * sc * sj1 * sc1
                lf2[j1] = lfj1 + 2 * sg
                lf2[jc1] = lfc1 + 2 * sg
                lfc += 2 * sg
            lf2[jc] = lfc
        else:
            for y in Ux:
                lfy = lf2[y]
                ll2[y] = lfy
                lf2[y] = -lfy
            sc = 2 * int(s[jc]) - 1
            for Ux1 in Us:
                jc1 = Ux1[0]
                lfc1 = lf2[jc1]
                ll2[jc1] = lfc1
                sc1 = 2 * int(s[jc1]) - 1
                for j1 in range(jc1 + 1, Ux1[-1] + 1):
                    lfj1 = lf2[j1]
                    ll2[j1] = lfj1
                    sj1 = 2 * int(s[j1]) - 1
                    sx = 2 * int(s[jc + (j1 - jc1)]) - 1
                    sg = sx * sc * sj1 * sc1
                    lf2[j1] = lfj1 + 2 * sg
                    lfc1 += 2 * sg
                lf2[jc1] = lfc1
        self.move_last2 = move

    def delta(self, move):                   # TLE.jl:301-311: 2γT * lfields1 + 2λT * lfields2, in that order
        return (2 * self.gT) * self.lf1[move] + (2 * self.lT) * self.lf2[move]

    def neighbors(self, j):                  # TLE.jl:313-333
        M = self.M
        k = j % (M + 1)
        i = j // (M + 1)
        if k == 0:
            out = list(range(j + 1, j + M + 1))
            for i1 in self.neighb[i]:
                out.extend(range(i1 * (M + 1), (i1 + 1) * (M + 1)))
            return out
        out = [j - k]
        for i1 in self.neighb[i]:
            out.append(i1 * (M + 1))
            out.append(k + i1 * (M + 1))
        return out

    def fields_of(self, s):
        """(lfields1, lfields2) as the functions of the spins the issue's definition gives"""
        M, Nk = self.M, self.Nk
        sg = [2 * int(x) - 1 for x in s]
        o1, o2 = [0] * self.N, [0] * self.N
        for i in range(Nk):
            jc = i * (M + 1)
            o1[jc] = sg[jc] * sum(sg[jc + k] for k in range(1, M + 1))
            for k in range(1, M + 1):
                o1[jc + k] = sg[jc] * sg[jc + k]
                o2[jc + k] = sg[jc + k] * sg[jc] * sum(sg[i2 * (M + 1)] * sg[i2 * (M + 1) + k] for i2 in self.neighb[i])
            o2[jc] = sg[jc] * sum(sg[i2 * (M + 1)] * sum(sg[jc + k] * sg[i2 * (M + 1) + k] for k in range(1, M + 1)) for i2 in self.neighb[i])
        return o1, o2


def neighb_of(kind, Nk, sat=None):
    """∂i = neighbors(g0, i) of the slice graph: empty (GraphEmpty), AllButOne (GraphSK / GraphSKNormal), neighb[i] (GraphSAT)"""
    if kind == "empty":
        return [[] for _ in range(Nk)]
    if kind == "sat":
        return [list(ni) for ni in SR.ClauseCache(*sat).neighb]
    return [[j for j in range(Nk) if j != i] for i in range(Nk)]


class TopologicalLocalEntropy(LE.LocalEntropy):
    """GraphTopologicalLocalEntropy{M,γT,λT,G} (TLE.jl:351-502): LocalEntropy's DoubleGraph (update_cache!, energy, residual are LE's text)
    over X0 = GraphTLE; ``sat`` = (N, A, J) for GraphSAT slices"""

    def __init__(self, Nk, M, gamma, lam, beta, kind, J=None, sat=None, neighb=None):
        self.Nk, self.M, self.gamma, self.lam, self.beta, self.kind, self._Jc, self._sat = Nk, M, gamma, lam, beta, kind, J, sat
        self.gT, self.lT = gamma / beta, lam / beta                     # TLE.jl:390-396
        self.N = Nk * (M + 1)
        self.neighb = neighb_of(kind, Nk, sat) if neighb is None else neighb
        self.X0 = GraphTLE(Nk, M, self.gT, self.lT, self.neighb)
        if kind == "sat":
            self.Xc = SR.SatRef(*sat)
            self.X1 = [SR.SatRef(*sat) for _ in range(M)]
        else:
            self.Xc = make_slices(kind, Nk, 1, J)[0]
            self.X1 = make_slices(kind, Nk, M, J)
        self.Cc = np.zeros(Nk, np.int64)
        self.C1 = [np.zeros(Nk, np.int64) for _ in range(M)]
        self.ae = all_delta_e(M, self.gT, self.lT, self.X0.maxdeg)
        self.L = len(self.ae)

    def fresh(self):
        return TopologicalLocalEntropy(self.Nk, self.M, self.gamma, self.lam, self.beta, self.kind, self._Jc, self._sat, self.neighb)


def energy_fresh(X, s):
    """energy(X, C) of a fresh graph object (does not disturb a running one)"""
    return X.fresh().energy(np.array(s, np.int64))


def slice_of(X):
    return SR.SatRef(*X._sat) if X.kind == "sat" else make_slices(X.kind, X.Nk, 1, X._Jc)[0]


def tle_energies(X, s):
    """TLEenergies (TLE.jl:437-453) of configuration s, a fresh slice per replica"""
    return [float(slice_of(X).energy(np.asarray(s[k + 1::X.M + 1], np.int64))) for k in range(X.M)]


def cenergy(X, s):
    """cenergy (TLE.jl:455-458)"""
    return float(slice_of(X).energy(np.asarray(s[0::X.M + 1], np.int64)))


distances = LE.distances                 # TLE.jl:493-502 is LE.jl:309-318


class DeltaECache(RE.DeltaECache):
    """DeltaE.jl:74-103 over GraphTLE: findk on the Float64 ΔE0; 0-based classes a + L up"""

    def __init__(self, X, s, beta_s, det_exp):
        self.X = X
        self.ae = X.ae
        L = len(self.ae)
        self.L = L
        self.sets = [ArraySet(X.N) for _ in range(2 * L)]
        self.pos = [0] * X.N
        for j in range(X.N):
            self.pos[j] = self.classify(j, s)
            self.sets[self.pos[j]].push(j)
        self.ft = [det_exp(-beta_s * dE) for dE in self.ae]
        self.T = [0.0] * (2 * L)
        self.z = 0.0
        for k in range(2 * L):
            x = self.sets[k].t * self.f(k)
            self.z += x
            self.T[k] = x

    def classify(self, j, s):
        dE = self.X.X0.delta(j)
        a = findk(self.ae, dE)
        assert a > 0, (j, dE)
        up = dE > 0 or (dE == 0 and s[j] == 1)
        return (a - 1) + self.L * up


class RrrRun(RE.RrrRun):
    """rrrMC(X::DoubleGraph) (RRRMC.jl:221-290) as a resumable chain: re_reference's loop over the TLE graph and its cache"""

    def __init__(self, X, s, beta, seed, oracle, replica=0, it0=0, staged_thr=0.5, staged_thr_fact=5.0):
        self.X, self.s, self.beta, self.seed, self.O, self.rep = X, s, beta, seed, oracle, replica
        self.E = X.energy(s)
        self.cache = DeltaECache(X, s, beta, oracle.det_exp)
        self.lam = staged_thr_fact / X.N
        self.staged_thr = staged_thr
        self.acc_rate = 0.5
        self.it = 0
        self.g0 = it0
        self.accepted = 0
        self.staged_its = 0
        self.check_E = False

    def cache_view(self):
        return np.array(self.cache.pos, np.int32), np.array([a.t for a in self.cache.sets], np.int32)


standard_mc = LE.standard_mc
