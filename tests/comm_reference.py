"""Plain-Python restatement of the reference's binary committee machines, written from src/graphs/CommStep.jl and src/graphs/CommReLU.jl
(line numbers below are theirs).  The Stabilities keep literal ArraySets (``re_reference.ArraySet``), as the reference does; the ξsi /
last_move copy of one pattern column (CommStep.jl:153) is an access optimisation and is read straight from ξ here.  Units and patterns are
0-based: unit k owns synapses k K1 .. (k + 1) K1 - 1.

A ``CommStepRef`` / ``CommReLURef`` is usable as a slice class by ``re_reference`` and ``le_reference`` (energy, delta, flip_update), as
``perc_reference``'s classes are: ``re_ensemble`` / ``le_ensemble`` put M committee machines that share one pattern matrix in place of the
GraphEmpty slices (src/REAliases.jl:126-166, src/LEAliases.jl).  Configurations are 0/1 integer arrays (1 = +1); labels y are 0/1."""
import numpy as np

import le_reference as LE
import re_reference as RE
from re_reference import ArraySet


def sign(x):
    return (x > 0) - (x < 0)


class CommStepRef:
    """GraphCommStep (CommStep.jl:50-71): ET = Int"""
    relu = False

    def __init__(self, K2, xi, y=None):
        xi = np.asarray(xi, np.int64)
        self.P, self.N = xi.shape
        assert self.N % K2 == 0                                        # :61
        self.K2, self.K1 = K2, self.N // K2
        if self.K1 % 2 == 0:
            raise ValueError("K1 must be odd, given: %d" % self.K1)    # :65
        if K2 % 2 == 0:
            raise ValueError("K2 must be odd, given: %d" % K2)         # :66
        assert y is None
        self.xi = xi
        self._empty()

    def _empty(self):                                                  # empty! (:95-105)
        self.p1 = [ArraySet(self.P) for _ in range(self.K2)]
        self.m1 = [ArraySet(self.P) for _ in range(self.K2)]
        self.p2, self.m2 = ArraySet(self.P), ArraySet(self.P)
        self.d1 = [[0] * self.P for _ in range(self.K2)]
        self.d2 = [0] * self.P

    def _unit(self, s, k, a):
        K1 = self.K1
        return K1 - 2 * int((np.asarray(s)[k * K1:(k + 1) * K1] ^ self.xi[a, k * K1:(k + 1) * K1]).sum())

    def energy(self, s):                                               # :107-141
        E = 0
        self._empty()
        for a in range(self.P):
            D2 = 0
            for k in range(self.K2):
                D1 = self._unit(s, k, a)
                self.d1[k][a] = D1
                D2 += sign(D1)
                if D1 == 1:
                    self.p1[k].push(a)
                elif D1 == -1:
                    self.m1[k].push(a)
            self.d2[a] = D2
            if D2 == 1:
                self.p2.push(a)
            elif D2 < 0:
                if D2 == -1:
                    self.m2.push(a)
                E += 1
        return E

    def flip_update(self, s, move):                                    # update_cache! (:143-197), after the flip of s[move]
        si = int(s[move])
        k2 = move // self.K1
        D1k, p1k, m1k = self.d1[k2], self.p1[k2], self.m1[k2]
        for a in range(self.P):
            xsi = int(self.xi[a, move]) ^ si
            oldD2 = self.d2[a]
            oldD1 = D1k[a]
            newD1 = oldD1 + (2 - 4 * xsi)
            newD2 = oldD2
            if oldD1 > 1 and newD1 == 1:
                p1k.push(a)
            elif oldD1 == 1:
                p1k.delete(a)
                if newD1 == -1:
                    m1k.push(a)
                    newD2 -= 2
            elif oldD1 == -1:
                m1k.delete(a)
                if newD1 == 1:
                    p1k.push(a)
                    newD2 += 2
            elif oldD1 < -1 and newD1 == -1:
                m1k.push(a)
            D1k[a] = newD1
            if newD2 == oldD2:
                continue
            if oldD2 > 1 and newD2 == 1:
                self.p2.push(a)
            elif oldD2 == 1:
                self.p2.delete(a)
                if newD2 == -1:
                    self.m2.push(a)
            elif oldD2 == -1:
                self.m2.delete(a)
                if newD2 == 1:
                    self.p2.push(a)
            elif oldD2 < -1 and newD2 == -1:
                self.m2.push(a)
            self.d2[a] = newD2

    def delta(self, s, move):                                          # delta_energy (:212-242)
        si = int(s[move])
        k2 = move // self.K1
        p1 = set(self.p1[k2].v[:self.p1[k2].t])
        m1 = set(self.m1[k2].v[:self.m1[k2].t])
        dE = 0
        for a in self.p2.v[:self.p2.t]:
            if a in p1:
                dE += 1 - (int(self.xi[a, move]) ^ si)
        for a in self.m2.v[:self.m2.t]:
            if a in m1:
                dE -= int(self.xi[a, move]) ^ si
        return dE

    def sets(self):
        """(p1, m1, p2, m2) as Python sets of members"""
        f = lambda A: set(A.v[:A.t])                                   # noqa: E731
        return [f(A) for A in self.p1], [f(A) for A in self.m1], f(self.p2), f(self.m2)

    def check_sets(self):
        for A in self.p1 + self.m1 + [self.p2, self.m2]:
            A.check()


class CommReLURef(CommStepRef):
    """GraphCommReLU (CommReLU.jl:51-74): ET = Int"""
    relu = True

    def __init__(self, K2, xi, y):
        xi = np.asarray(xi, np.int64)
        self.P, self.N = xi.shape
        assert self.N % K2 == 0                                        # :63
        self.K2, self.K1 = K2, self.N // K2
        assert y is not None and len(y) == self.P                      # :67
        if self.K1 % 2 != 0:
            raise ValueError("K1 must be even, given: %d" % self.K1)   # :68
        if K2 % 2 != 0:
            raise ValueError("K2 must be even, given: %d" % K2)        # :69
        self.xi, self.y = xi, [int(v) for v in y]
        self._empty()

    def c(self, k):                                                    # 0-based unit k: c = 2 (2(k+1) <= K2) - 1 (:124)
        return 1 if 2 * (k + 1) <= self.K2 else -1

    def energy(self, s):                                               # :111-147
        E = 0
        self._empty()
        for a in range(self.P):
            D2 = 0
            for k in range(self.K2):
                D1 = self._unit(s, k, a)
                self.d1[k][a] = D1
                D2 += self.c(k) * max(D1, 0)
                if D1 > 0:
                    self.p1[k].push(a)
                elif D1 == 0:
                    self.m1[k].push(a)
            D2 *= 2 * self.y[a] - 1
            self.d2[a] = D2
            if D2 == 2:
                self.p2.push(a)
            elif D2 <= 0:
                if D2 == 0:
                    self.m2.push(a)
                E += 1
        return E

    def flip_update(self, s, move):                                    # :149-214
        si = int(s[move])
        k2 = move // self.K1
        D1k, p1k, m1k = self.d1[k2], self.p1[k2], self.m1[k2]
        c = self.c(k2)
        for a in range(self.P):
            o = 2 * self.y[a] - 1
            oldD2 = self.d2[a] * o
            oldD1 = D1k[a]
            newD1 = oldD1 + (2 - 4 * (int(self.xi[a, move]) ^ si))
            newD2 = oldD2
            if oldD1 <= 0 and newD1 > 0:
                assert oldD1 == 0 and newD1 == 2
                m1k.delete(a)
                p1k.push(a)
                newD2 += 2 * c
            elif oldD1 > 0 and newD1 <= 0:
                assert oldD1 == 2 and newD1 == 0
                p1k.delete(a)
                m1k.push(a)
                newD2 -= 2 * c
            elif oldD1 > 0 and newD1 > 0:
                newD2 += c * (newD1 - oldD1)
            elif oldD1 < 0 and newD1 == 0:
                m1k.push(a)
            elif oldD1 == 0:
                assert newD1 < 0
                m1k.delete(a)
            D1k[a] = newD1
            if newD2 == oldD2:
                continue
            oldD2 *= o
            newD2 *= o
            if oldD2 > 2 and newD2 == 2:
                self.p2.push(a)
            elif oldD2 == 2:
                self.p2.delete(a)
                if newD2 == 0:
                    self.m2.push(a)
            elif oldD2 == 0:
                self.m2.delete(a)
                if newD2 == 2:
                    self.p2.push(a)
            elif oldD2 < 0 and newD2 == 0:
                self.m2.push(a)
            self.d2[a] = newD2

    def delta(self, s, move):                                          # :229-266
        si = int(s[move])
        k2 = move // self.K1
        c = self.c(k2)
        p1 = set(self.p1[k2].v[:self.p1[k2].t])
        m1 = set(self.m1[k2].v[:self.m1[k2].t])
        dE = 0
        for a in self.p2.v[:self.p2.t]:
            o = 2 * self.y[a] - 1
            x = int(self.xi[a, move]) ^ si
            if c == o and a in p1:
                dE += 1 - x
            elif c != o and (a in m1 or a in p1):
                dE += x
        for a in self.m2.v[:self.m2.t]:
            o = 2 * self.y[a] - 1
            x = int(self.xi[a, move]) ^ si
            if c == o and (a in m1 or a in p1):
                dE -= x
            elif c != o and a in p1:
                dE -= 1 - x
        return dE


def make(K2, xi, y=None):
    return (CommStepRef if y is None else CommReLURef)(K2, xi, y)


def masks_of(X):
    """what the engine keeps instead of the ArraySets: membership as a function of Δ1 / Δ2 (csrc/comm_kernels.hpp)"""
    if X.relu:
        p1 = [{a for a, d in enumerate(row) if d > 0} for row in X.d1]
        m1 = [{a for a, d in enumerate(row) if d == 0} for row in X.d1]
        p2 = {a for a, d in enumerate(X.d2) if d == 2}
        m2 = {a for a, d in enumerate(X.d2) if d == 0}
    else:
        p1 = [{a for a, d in enumerate(row) if d == 1} for row in X.d1]
        m1 = [{a for a, d in enumerate(row) if d == -1} for row in X.d1]
        p2 = {a for a, d in enumerate(X.d2) if d == 1}
        m2 = {a for a, d in enumerate(X.d2) if d == -1}
    return p1, m1, p2, m2


def delta_from_masks(X, s, move):
    """the engine's popcount rows (csrc/comm_kernels.hpp), restated on sets: col = the pattern column of `move` XOR its spin"""
    p1, m1, p2, m2 = masks_of(X)
    k2 = move // X.K1
    col = {a for a in range(X.P) if int(X.xi[a, move]) ^ int(s[move])}
    ncol = set(range(X.P)) - col
    A, Z = p1[k2], m1[k2]
    if not X.relu:
        return len(p2 & A & ncol) - len(m2 & Z & col)
    eq = {a for a in range(X.P) if X.y[a] == (1 if X.c(k2) > 0 else 0)}
    ne = set(range(X.P)) - eq
    AZ = A | Z
    return len(p2 & eq & A & ncol) + len(p2 & ne & AZ & col) - len(m2 & eq & AZ & col) - len(m2 & ne & A & ncol)


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
        if y is None:
            E += sum(np.sign(h)) < 0
        else:
            out = sum((1 if 2 * (k + 1) <= K2 else -1) * max(h[k], 0) for k in range(K2))
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


def standard_mc(X, s, beta, iters, step, seed, oracle, replica=0, it0=0, E=None):
    """standardMC (RRRMC.jl:81-127) on a stand-alone committee machine.  E = None: a fresh call (E = energy(X, C))"""
    if E is None:
        E = X.energy(s)
    Es, accepted = [], 0
    for it in range(1, iters + 1):
        if it % step == 0:
            Es.append(E)
        g = it0 + it
        move = oracle.site_of(seed, g, X.N)
        dE = X.delta(s, move)
        x = -beta * dE
        if not (x >= 0 or oracle.rand53(seed, g, replica) < oracle.det_exp(x)):
            continue
        s[move] ^= 1
        X.flip_update(s, move)
        E += dE
        accepted += 1
    return Es, E, accepted
