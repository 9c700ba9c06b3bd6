"""Plain-Python restatement of the reference's third binary committee machine, written from src/graphs/CommQu.jl (line numbers below are
its).  The Stabilities keep literal ArraySets p2 / m2 (``re_reference.ArraySet``) and, per pattern, the two extrema over the hidden units
that the reference holds in a MutableBinaryMaxHeap / MinHeap (:36-37): only ``first()`` of a heap is ever read (:144, :146, :184-185) and
``update!`` addresses an entry by the handle of its unit (:181-182), so a list per pattern read through ``max`` / ``min`` says the same.  The
ξsi / last_move copy of one pattern column (:164) is an access optimisation and is read straight from ξ here.  Units and patterns are 0-based:
unit k owns synapses k K1 .. (k + 1) K1 - 1.

A ``CommQuRef`` is usable as a slice class by ``re_reference``, ``le_reference`` and ``quant_pattern_reference`` (energy, delta,
flip_update), as ``comm_reference``'s classes are.  Configurations are 0/1 integer arrays (1 = +1); labels y are 0/1."""
import numpy as np

import le_reference as LE
import re_reference as RE
from comm_reference import standard_mc  # noqa: F401  (standardMC on a stand-alone machine: the same loop over energy / delta / flip_update)
from re_reference import ArraySet


class CommQuRef:
    """GraphCommQu (CommQu.jl:52-75): ET = Int"""

    def __init__(self, K2, xi, y):
        xi = np.asarray(xi, np.int64)
        self.P, self.N = xi.shape
        assert self.N % K2 == 0                                        # :64
        self.K2, self.K1 = K2, self.N // K2
        assert y is not None and len(y) == self.P                      # :68
        if self.K1 % 2 != 0:
            raise ValueError("K1 must be even, given: %d" % self.K1)   # :69
        if K2 % 2 != 0:
            raise ValueError("K2 must be even, given: %d" % K2)        # :70
        self.xi, self.y = xi, [int(v) for v in y]
        self._empty()

    def _empty(self):                                                  # empty! (:100-113)
        self.p2, self.m2 = ArraySet(self.P), ArraySet(self.P)
        self.d1 = [[0] * self.P for _ in range(self.K2)]               # Δ1s
        self.d2 = [0] * self.P                                         # Δ2s
        self.hmax = [[] for _ in range(self.P)]                        # δΔ2Hsmax[a]: entry k = the value pushed for unit k
        self.hmin = [[] for _ in range(self.P)]                        # δΔ2Hsmin[a]

    def c(self, k):                                                    # 0-based unit k: 2 (2(k+1) <= K2) - 1 (:131, :168)
        return 1 if 2 * (k + 1) <= self.K2 else -1

    def _unit(self, s, k, a):
        K1 = self.K1
        return K1 - 2 * int((np.asarray(s)[k * K1:(k + 1) * K1] ^ self.xi[a, k * K1:(k + 1) * K1]).sum())

    def energy(self, s):                                               # :115-152
        E = 0
        self._empty()
        for a in range(self.P):
            o = 2 * self.y[a] - 1
            D2 = 0
            hmax, hmin = [], []
            for k in range(self.K2):
                c = o * self.c(k)
                D1 = self._unit(s, k, a)
                self.d1[k][a] = D1
                D2 += c * D1 ** 2
                hmax.append(4 * (c + abs(c * D1)))                     # :137
                hmin.append(4 * (c - abs(c * D1)))                     # :138
            self.d2[a] = D2
            self.hmax[a], self.hmin[a] = hmax, hmin
            if D2 > 0:
                if D2 + min(hmin) <= 0:                                # :144
                    self.p2.push(a)
            else:
                if D2 + max(hmax) > 0:                                 # :146
                    self.m2.push(a)
                E += 1
        return E

    def flip_update(self, s, move):                                    # update_cache! (:154-206), after the flip of s[move]
        si = int(s[move])
        k2 = move // self.K1
        D1k = self.d1[k2]
        c = self.c(k2)
        p2m = set(self.p2.v[:self.p2.t])
        m2m = set(self.m2.v[:self.m2.t])
        for a in range(self.P):
            co = c * (2 * self.y[a] - 1)
            oldD2 = self.d2[a]
            oldD1 = D1k[a]
            newD1 = oldD1 + (2 - 4 * (int(self.xi[a, move]) ^ si))     # :174
            newD2 = oldD2 + co * (newD1 ** 2 - oldD1 ** 2)             # :176
            self.hmax[a][k2] = 4 * (co + abs(co * newD1))              # :181
            self.hmin[a][k2] = 4 * (co - abs(co * newD1))              # :182
            newmax, newmin = max(self.hmax[a]), min(self.hmin[a])
            oldm2 = a in m2m
            newm2 = newD2 <= 0 and newD2 + newmax > 0                  # :188
            oldp2 = a in p2m
            newp2 = newD2 > 0 and newD2 + newmin <= 0                  # :190
            if oldm2 and not newm2:
                self.m2.delete(a)
            if not oldm2 and newm2:
                self.m2.push(a)
            if oldp2 and not newp2:
                self.p2.delete(a)
            if not oldp2 and newp2:
                self.p2.push(a)
            D1k[a] = newD1
            self.d2[a] = newD2

    def _moved(self, s, move, a):
        """Δ2[a] after the flip of `move` (:240, :246)"""
        k2 = move // self.K1
        co = self.c(k2) * (2 * self.y[a] - 1)
        x = int(self.xi[a, move]) ^ int(s[move])
        return self.d2[a] + co * 4 * (1 - (1 - 2 * x) * self.d1[k2][a])

    def delta(self, s, move):                                          # delta_energy (:221-255)
        dE = 0
        for a in self.p2.v[:self.p2.t]:
            if self._moved(s, move, a) <= 0:
                dE += 1
        for a in self.m2.v[:self.m2.t]:
            if self._moved(s, move, a) > 0:
                dE -= 1
        return dE

    def sets(self):
        """(p2, m2) as Python sets of members"""
        return set(self.p2.v[:self.p2.t]), set(self.m2.v[:self.m2.t])

    def check_sets(self):
        self.p2.check()
        self.m2.check()

    def membership(self, a):
        """(in p2, in m2) by the reference's conditions (:144, :146, :188, :190) from the stabilities of pattern a"""
        D2 = self.d2[a]
        o = 2 * self.y[a] - 1
        hmax = max(4 * (o * self.c(k) + abs(self.d1[k][a])) for k in range(self.K2))
        hmin = min(4 * (o * self.c(k) - abs(self.d1[k][a])) for k in range(self.K2))
        return D2 > 0 and D2 + hmin <= 0, D2 <= 0 and D2 + hmax > 0


def make(K2, xi, y):
    return CommQuRef(K2, xi, y)


def delta_from_stabilities(X, s, move):
    """the engine's formula (csrc/comm_kernels.hpp): over ALL patterns, [Δ2 + t <= 0] − [Δ2 <= 0] with t = o_a c_u 4 (1 − (1 − 2x) Δ1[u][a]);
    pruned as the kernels prune, with the masks wrong = {Δ2 <= 0} and near = {|Δ2| <= 4 (1 + K1)}"""
    full = sum((X._moved(s, move, a) <= 0) - (X.d2[a] <= 0) for a in range(X.P))
    near = [a for a in range(X.P) if abs(X.d2[a]) <= 4 * (1 + X.K1)]
    wrong = {a for a in range(X.P) if X.d2[a] <= 0}
    pruned = sum(X._moved(s, move, a) <= 0 for a in near) - len(wrong & set(near))
    assert full == pruned
    return full


def energy_from_definition(K2, xi, y, s):
    """the number of misclassified patterns from the model's definition, with ±1 spins and patterns (no caches)"""
    xi = np.asarray(xi, np.int64)
    P, N = xi.shape
    K1 = N // K2
    sg = 2 * np.asarray(s, np.int64) - 1
    xg = 2 * xi - 1
    E = 0
    for a in range(P):
        h = [int((sg[k * K1:(k + 1) * K1] * xg[a, k * K1:(k + 1) * K1]).sum()) for k in range(K2)]
        out = sum((1 if 2 * (k + 1) <= K2 else -1) * h[k] ** 2 for k in range(K2))
        E += out * (2 * int(y[a]) - 1) <= 0
    return int(E)


def re_ensemble(K2, xi, y, M, gamma, beta):
    Nk = np.asarray(xi).shape[1]
    X = RE.make_ensemble(Nk, M, gamma, beta, "empty")
    X.X1 = [make(K2, xi, y) for _ in range(M)]
    return X


def le_ensemble(K2, xi, y, M, gamma, beta):
    Nk = np.asarray(xi).shape[1]
    X = LE.make_ensemble(Nk, M, gamma, beta, "empty")
    X.Xc = make(K2, xi, y)
    X.X1 = [make(K2, xi, y) for _ in range(M)]
    return X


def quant_reference(X):
    """the quant_pattern_reference object of a product GraphQCommQuT: its slices from the public pattern arrays"""
    import quant_pattern_reference as QR
    X1 = X.X1
    xi, y = X1.patterns(), X1.labels()
    return QR.GraphQuantRef(X.Nk, X.M, X.fourK, [make(X1.K2, xi, y) for _ in range(X.M)])
