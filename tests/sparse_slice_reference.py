"""Plain-Python restatement of a sparse Float64 slice graph — GraphEANormal (src/graphs/EA.jl:534-680; GraphRRGNormal's text, RRG.jl:503-617,
is the same) — TEST INFRASTRUCTURE for the ensembles over it (GraphEARE, GraphEALE, GraphEATLE: src/REAliases.jl:43-75, src/LEAliases.jl:43-75,
src/TLEAliases.jl:36-68), written from the Julia sources, not from the HIP code.

``SliceSparseF64(A, J)`` has the interface of the slice classes of tests/re_reference.py (``energy``, ``delta``, ``flip_update``) and ``neighb``,
the lists ``uA`` that ``neighbors(g0, i)`` returns (EA.jl:680).  The helpers below build the RE, LE and TLE reference objects of
re_reference.py / le_reference.py / tle_reference.py around it: those modules are used as they are, constructed over GraphEmpty slices, with
the slices (and the TLE neighbour lists) replaced."""
import numpy as np

import le_reference as LE
import re_reference as RE
import tle_reference as TLE


class SliceSparseF64:
    """A [Nk][K] 0-based neighbour table with ascending rows (a neighbour may repeat: L = 2), J [Nk][K] Float64.  The cache is the reference's
    LocalFields{Float64}: lfields, lfields_last (all Nk entries, as the reference keeps them) and move_last."""

    def __init__(self, A, J):
        self.A = [[int(y) for y in row] for row in np.asarray(A)]
        self.J = [[float(x) for x in row] for row in np.asarray(J, np.float64)]
        self.Nk = len(self.A)
        self.K = len(self.A[0])
        self.uA = []
        for row in self.A:                       # unique(a), first appearances in order (EA.jl:548)
            u = []
            for y in row:
                if y not in u:
                    u.append(y)
            self.uA.append(u)
        self.neighb = self.uA                    # neighbors(X, i) = X.uA[i] (EA.jl:680)
        self.lf = [0.0] * self.Nk
        self.lfl = [0.0] * self.Nk
        self.move_last = -1

    def energy(self, s):                         # EA.jl:584-611
        E1 = 0.0
        for x in range(self.Nk):
            Jx, Ax = self.J[x], self.A[x]
            sx = 2 * int(s[x]) - 1
            lf = 0.0
            for k in range(len(Ax)):
                sy = 2 * int(s[Ax[k]]) - 1
                lf -= Jx[k] * sx * sy
            E1 += lf
            self.lf[x] = 2 * lf
        E1 /= 2
        self.move_last = -1
        self.lfl = [0.0] * self.Nk
        return E1

    def delta(self, s, i):                       # EA.jl:655-663
        return -self.lf[i]

    def flip_update(self, s, i):                 # update_cache! after the flip of s[i] (EA.jl:613-653)
        lf, lfl = self.lf, self.lfl
        if self.move_last == i:
            for y in self.uA[i]:
                lf[y], lfl[y] = lfl[y], lf[y]
            lf[i] = -lf[i]
            lfl[i] = -lfl[i]
            return
        for y in self.uA[i]:
            lfl[y] = lf[y]
        Jx, Ax = self.J[i], self.A[i]
        sx = int(s[i])
        for k in range(len(Ax)):                 # a neighbour listed twice receives both bonds, in row order
            y = Ax[k]
            sxy = 1 - 2 * (sx ^ int(s[y]))
            lf[y] -= 4 * sxy * Jx[k]
        lfm = lf[i]
        lfl[i] = lfm
        lf[i] = -lfm
        self.move_last = i


def brute_energy(A, J, s):
    """-Σ_bonds J σx σy from the definition: every table entry is half a bond; exact summation (math.fsum), for the CPU checks"""
    import math
    terms = []
    for x in range(len(A)):
        for k in range(len(A[x])):
            terms.append(-float(J[x][k]) * (2 * int(s[x]) - 1) * (2 * int(s[int(A[x][k])]) - 1))
    return math.fsum(terms) / 2


def slices(A, J, M):
    return [SliceSparseF64(A, J) for _ in range(M)]


def make_re(A, J, M, gamma, beta):
    """GraphRobustEnsemble(Nk, M, γ, β, GraphEANormal{K}, L, A, J)"""
    X = RE.make_ensemble(len(A), M, gamma, beta, "empty")
    X.X1 = slices(A, J, M)
    X.kind, X._Jc = "sparse_f64", (A, J)
    return X


def make_le(A, J, M, gamma, beta):
    """GraphLocalEntropy(Nk, M, γ, β, GraphEANormal{K}, L, A, J): the centre graph and the M slices"""
    X = LE.make_ensemble(len(A), M, gamma, beta, "empty")
    X.Xc = SliceSparseF64(A, J)
    X.X1 = slices(A, J, M)
    X.kind, X._Jc = "sparse_f64", (A, J)
    return X


def make_tle(A, J, M, gamma, lam, beta):
    """GraphTopologicalLocalEntropy(Nk, M, γ, λ, β, GraphEANormal{K}, L, A, J): ∂i = neighbors(g0, i) = uA[i] (TLE.jl:394)"""
    g0 = SliceSparseF64(A, J)
    X = TLE.TopologicalLocalEntropy(len(A), M, gamma, lam, beta, "empty", neighb=[list(u) for u in g0.neighb])
    X.Xc = g0
    X.X1 = slices(A, J, M)
    X.kind, X._Jc = "sparse_f64", (A, J)
    return X


def slice_energy(A, J, srow):
    """energy(X1, C1) of a fresh slice for the configuration srow"""
    return float(SliceSparseF64(A, J).energy(np.asarray(srow, np.int64)))


def re_energies(A, J, M, s):
    return [slice_energy(A, J, s[k::M]) for k in range(M)]


def le_energies(A, J, M, s):                     # LEenergies / TLEenergies
    return [slice_energy(A, J, s[k + 1::M + 1]) for k in range(M)]


def cenergy(A, J, M, s):
    return slice_energy(A, J, s[0::M + 1])
