"""Plain-Python restatement of the Local Entropy ensemble — TEST INFRASTRUCTURE, written from the Julia sources (src/graphs/LE.jl,
src/LEAliases.jl, src/Interface.jl:273-287, src/RRRMC.jl:81-127 and :221-290, src/DeltaE.jl:26-295), not from the HIP code.

The generic pieces come from ``re_reference.py`` (ArraySet, the slice graphs, the DeltaECache's class weights and consistency check, the
rrrMC loop, the stream draws).  What is LE's own is restated literally here: GraphLE's integer LocalFields with update_cache!'s move_last
swap (LE.jl:55-154), findk's generated binary search (DeltaE.jl:26-60) on the Float64 ΔE, the DoubleGraph's update_cache! (the centre's
graph cache is not updated, LE.jl:227-240), energy (the centre's own energy is not part of it), and the observables.
Sites are 0-based: site j is spin i = j // (M+1) of the centre when j % (M+1) == 0, of replica j % (M+1) otherwise (LE.jl:55-84)."""
import numpy as np

import re_reference as RE
from re_reference import ArraySet, chunks_from_config, config_from_chunks, make_slices, rrr_draws  # noqa: F401


# ---- GraphLE{M,γT} (LE.jl:17-179) ----------------------------------------------------------------------------------------------
def gamma_t(gamma, beta):
    return gamma / beta                      # LE.jl:221-225: a Float64 division, once


def all_delta_e(M, gT):
    """allΔE(GraphLE{M,γT}) (LE.jl:176-179)"""
    if M % 2 == 0:
        lst = [4 * d * abs(gT) for d in range(M // 2 + 1)]
        lst.insert(1, 2 * abs(gT))
        return lst
    return [2 * (2 * d - 1) * abs(gT) for d in range(1, (M + 1) // 2 + 1)]


def findk(dElist, dE):
    """findk (DeltaE.jl:26-60) as the generated code runs: 1-based, 0 when absent"""
    dE = abs(dE)

    def search(imin, imax, i):
        if imax - imin < 10:
            for j in range(imin, imax + 1):
                if dE == dElist[j - 1]:
                    return j
            return 0
        cE = dElist[i - 1]
        if cE == dE:
            return i
        if cE < dE:
            return search(i + 1, imax, (i + 1 + imax) // 2)
        return search(imin, i - 1, (imin + i - 1) // 2)

    L = len(dElist)
    return search(1, L, (1 + L) // 2)


class GraphLE:
    """the inner graph: LocalFields{Int} (lfields, lfields_last, move_last; -1 = none)"""

    def __init__(self, Nk, M, gT):
        self.Nk, self.M, self.gT = Nk, M, gT
        self.N = Nk * (M + 1)
        self.lfields = [0] * self.N
        self.lfields_last = [0] * self.N
        self.move_last = -1

    def energy(self, s):                     # LE.jl:55-84
        M = self.M
        n = 0
        j = -1
        for i in range(self.Nk):
            j += 1
            jc = j
            sc = 2 * int(s[jc]) - 1
            mu = 0
            for k in range(1, M + 1):
                j += 1
                sj = 2 * int(s[j]) - 1
                self.lfields[j] = sc * sj
                mu += sj
            f = sc * mu
            self.lfields[jc] = f
            n -= f
        self.move_last = -1
        self.lfields_last = [0] * self.N
        return n * self.gT

    def kinterval(self, move):               # LE.jl:86-90
        j0 = move - move % (self.M + 1)
        return range(j0, j0 + self.M + 1)

    def update_cache(self, s, move):         # LE.jl:92-154, after the flip of s[move]
        M = self.M
        k = move % (M + 1)
        lf, ll = self.lfields, self.lfields_last
        if k != 0:
            sx = 2 * int(s[move]) - 1
            i = move // (M + 1)
            jc = i * (M + 1)
        else:
            Ux = self.kinterval(move)
        if self.move_last == move:
            if k != 0:
                lf[jc], ll[jc] = ll[jc], lf[jc]
                lf[move], ll[move] = ll[move], lf[move]
            else:
                for y in Ux:
                    lf[y], ll[y] = ll[y], lf[y]
            return
        if k != 0:
            sc = 2 * int(s[jc]) - 1
            lfc = lf[jc]
            lfm = lf[move]
            ll[jc] = lfc
            ll[move] = lfm
            lf[jc] = lfc + 2 * (sc * sx)
            lf[move] = -lfm
        else:
            for y in Ux:
                lfy = lf[y]
                ll[y] = lfy
                lf[y] = -lfy
        self.move_last = move

    def delta(self, move):                   # LE.jl:156-164
        return 2 * self.gT * self.lfields[move]

    def neighbors(self, j):                  # LE.jl:166-174
        r = j % (self.M + 1)
        if r == 0:
            return list(range(j + 1, j + self.M + 1))
        return [j - r]

    def fields_of(self, s):
        """lfields as the function of the spins that update_cache! is claimed to keep"""
        M = self.M
        out = [0] * self.N
        for i in range(self.Nk):
            jc = i * (M + 1)
            sc = 2 * int(s[jc]) - 1
            mu = sum(2 * int(s[jc + k]) - 1 for k in range(1, M + 1))
            out[jc] = sc * mu
            for k in range(1, M + 1):
                out[jc + k] = sc * (2 * int(s[jc + k]) - 1)
        return out


# ---- GraphLocalEntropy{M,γT,G} (LE.jl:183-318) -----------------------------------------------------------------------------------
class LocalEntropy:
    """X0 = GraphLE, Xc = the centre graph, X1 = the M slices, Cc / C1 their configurations"""

    def __init__(self, Nk, M, gamma, beta, kind, J=None):
        if M <= 2:
            raise ValueError("M must be greater than 2")
        self.Nk, self.M, self.gamma, self.beta, self.kind, self._Jc = Nk, M, gamma, beta, kind, J
        self.gT = gamma_t(gamma, beta)
        self.N = Nk * (M + 1)
        self.X0 = GraphLE(Nk, M, self.gT)
        self.Xc = make_slices(kind, Nk, 1, J)[0]
        self.X1 = make_slices(kind, Nk, M, J)
        self.Cc = np.zeros(Nk, np.int64)
        self.C1 = [np.zeros(Nk, np.int64) for _ in range(M)]
        self.L = len(all_delta_e(M, self.gT))

    def energy(self, s):                     # LE.jl:242-258
        M = self.M
        E = self.X0.energy(s)
        self.Cc[:] = s[0::M + 1]
        self.Xc.energy(self.Cc)
        for k in range(M):
            self.C1[k][:] = s[k + 1::M + 1]
            E += self.X1[k].energy(self.C1[k])
        return E

    def spinflip0(self, s, move):            # spinflip!(X0, C, move)
        s[move] ^= 1
        self.X0.update_cache(s, move)

    def spinflip(self, s, move):             # spinflip!(X, C, move): update_cache! of LE.jl:227-240
        s[move] ^= 1
        k, i = move % (self.M + 1), move // (self.M + 1)
        if k == 0:
            self.Cc[i] ^= 1                  # the centre graph's cache is not updated
        else:
            self.C1[k - 1][i] ^= 1
            self.X1[k - 1].flip_update(self.C1[k - 1], i)
        self.X0.update_cache(s, move)

    def residual(self, move):                # LE.jl:276-290: not divided by M
        k = move % (self.M + 1)
        if k == 0:
            return 0.0
        i = move // (self.M + 1)
        return self.X1[k - 1].delta(self.C1[k - 1], i)

    def delta(self, move):                   # LE.jl:292-295
        return self.X0.delta(move) + self.residual(move)

    def neighbors0(self, move):
        return self.X0.neighbors(move)


def make_ensemble(Nk, M, gamma, beta, kind, J=None):
    return LocalEntropy(Nk, M, gamma, beta, kind, J)


def energy_fresh(Nk, M, gamma, beta, kind, J, s):
    """energy(X, C) of a fresh graph object (does not disturb a running one)"""
    return make_ensemble(Nk, M, gamma, beta, kind, J).energy(np.array(s, np.int64))


def le_energies(Nk, M, kind, J, s):
    """LEenergies (LE.jl:259-269) of configuration s, a fresh slice per replica"""
    return [float(make_slices(kind, Nk, 1, J)[0].energy(np.asarray(s[k + 1::M + 1], np.int64))) for k in range(M)]


def cenergy(Nk, M, kind, J, s):
    """cenergy (LE.jl:271-274): the centre configuration under the slice graph"""
    return float(make_slices(kind, Nk, 1, J)[0].energy(np.asarray(s[0::M + 1], np.int64)))


def distances(Nk, M, s):
    """distances (LE.jl:309-318): Hamming distances of the replica configurations"""
    rows = [np.asarray(s[k + 1::M + 1], np.int64) for k in range(M)]
    return [[int((rows[a] ^ rows[b]).sum()) for b in range(M)] for a in range(M)]


# ---- DeltaECache and rrrMC ------------------------------------------------------------------------------------------------------
class DeltaECache(RE.DeltaECache):
    """DeltaE.jl:74-103 over GraphLE: findk on the Float64 ΔE0 = 2γT lfields; 0-based classes a + L up"""

    def __init__(self, X, s, beta_s, det_exp):
        self.X = X
        self.ae = all_delta_e(X.M, X.gT)
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
    """rrrMC(X::DoubleGraph) (RRRMC.jl:221-290) as a resumable chain: re_reference's loop (rand_move, compute_staged! through two flips of X0,
    apply_staged!, apply_move!) over the LE graph and its cache"""

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
        dE = X.delta(move)
        x = -beta * dE
        if not (x >= 0 or oracle.rand53(seed, g, replica) < oracle.det_exp(x)):
            continue
        X.spinflip(s, move)
        E += dE
        accepted += 1
    return Es, E, accepted
