"""Plain-Python restatement of the reference's binary perceptron graphs, written from src/graphs/PercStep.jl and src/graphs/PercLinear.jl
(line numbers below are theirs).  The Stabilities keep literal ArraySets (``re_reference.ArraySet``), as the reference does; the ξsi /
last_move copy of one pattern column (PercStep.jl:120-123) is an access optimisation and is read straight from ξ here.

A ``PercStepRef`` / ``PercLinearRef`` is usable as a slice class by ``re_reference`` and ``le_reference`` (energy, delta, flip_update):
``re_ensemble`` / ``le_ensemble`` build their ensembles over GraphEmpty and put M perceptrons that share one pattern matrix in its place,
as ``Gconstr(args...)`` with ``X.ξ, X.ξv`` does (src/REAliases.jl, src/LEAliases.jl).  Configurations are 0/1 integer arrays (1 = +1)."""
import math

import numpy as np

import le_reference as LE
import re_reference as RE
from re_reference import ArraySet


class PercStepRef:
    """GraphPercStep (PercStep.jl:44-72): ET = Int"""
    linear = False

    def __init__(self, xi):
        xi = np.asarray(xi, np.int64)
        self.P, self.N = xi.shape
        if self.N % 2 == 0:
            raise ValueError("N must be odd, given: %d" % self.N)      # :57
        self.xi = xi
        self.p, self.m = ArraySet(self.P), ArraySet(self.P)            # Stabilities (:31-43)
        self.ds = [0] * self.P
        self.sN = math.sqrt(self.N)

    def _empty(self):                                                  # empty! (:74-81)
        self.p, self.m = ArraySet(self.P), ArraySet(self.P)
        self.ds = [0] * self.P

    def energy(self, s):                                               # :83-111
        E = 0
        self._empty()
        for a in range(self.P):
            d = self.N - 2 * int((np.asarray(s) ^ self.xi[a]).sum())
            self.ds[a] = d
            if d == 1:
                self.p.push(a)
            elif d < 0:
                if d == -1:
                    self.m.push(a)
                E += 1
        return E

    def flip_update(self, s, i):                                       # update_cache! (:113-143), after the flip of s[i]
        si = int(s[i])
        for a in range(self.P):
            xsi = int(self.xi[a, i]) ^ si
            old = self.ds[a]
            new = old + (2 - 4 * xsi)
            if old > 1 and new == 1:
                self.p.push(a)
            elif old == 1:
                self.p.delete(a)
                if new == -1:
                    self.m.push(a)
            elif old == -1:
                self.m.delete(a)
                if new == 1:
                    self.p.push(a)
            elif old < -1 and new == -1:
                self.m.push(a)
            self.ds[a] = new

    def delta(self, s, i):                                             # delta_energy (:150-173)
        si = int(s[i])
        dE = 0
        for a in self.p.v[:self.p.t]:
            dE += 1 - (int(self.xi[a, i]) ^ si)
        for a in self.m.v[:self.m.t]:
            dE -= int(self.xi[a, i]) ^ si
        return dE

    def members(self):
        return set(self.p.v[:self.p.t]), set(self.m.v[:self.m.t])


class PercLinearRef(PercStepRef):
    """GraphPercLinear (PercLinear.jl:44-75): ET = Float64"""
    linear = True

    def energy(self, s):                                               # :83-115
        E = 0
        self._empty()
        for a in range(self.P):
            d = self.N - 2 * int((np.asarray(s) ^ self.xi[a]).sum())
            self.ds[a] = d
            if d == 1:
                self.p.push(a)
            elif d < 0:
                self.m.push(a)
                E += (-d - 1) // 2 + 1
        return 2 * E / self.sN

    def flip_update(self, s, i):                                       # :117-145
        si = int(s[i])
        for a in range(self.P):
            xsi = int(self.xi[a, i]) ^ si
            old = self.ds[a]
            new = old + (2 - 4 * xsi)
            if old > 1 and new == 1:
                self.p.push(a)
            elif old == 1:
                self.p.delete(a)
                if new < 0:
                    self.m.push(a)
            elif old < 0 and new == 1:
                self.m.delete(a)
                self.p.push(a)
            self.ds[a] = new

    def delta(self, s, i):                                             # :154-177
        si = int(s[i])
        dE = 0
        for a in self.p.v[:self.p.t]:
            dE += 1 - (int(self.xi[a, i]) ^ si)
        for a in self.m.v[:self.m.t]:
            dE -= 2 * (int(self.xi[a, i]) ^ si) - 1
        return 2 * dE / self.sN


def make(xi, linear):
    return (PercLinearRef if linear else PercStepRef)(xi)


def masks_of(ds, linear):
    """what the engine keeps instead of the ArraySets: membership as a function of Δ (csrc/perc_kernels.hpp)"""
    p = {a for a, d in enumerate(ds) if d == 1}
    m = {a for a, d in enumerate(ds) if (d < 0 if linear else d == -1)}
    return p, m


def re_ensemble(xi, linear, M, gamma, beta):
    Nk = np.asarray(xi).shape[1]
    X = RE.make_ensemble(Nk, M, gamma, beta, "empty")
    X.X1 = [make(xi, linear) for _ in range(M)]
    return X


def le_ensemble(xi, linear, M, gamma, beta):
    Nk = np.asarray(xi).shape[1]
    X = LE.make_ensemble(Nk, M, gamma, beta, "empty")
    X.Xc = make(xi, linear)
    X.X1 = [make(xi, linear) for _ in range(M)]
    return X


def standard_mc(X, s, beta, iters, step, seed, oracle, replica=0, it0=0, E=None):
    """standardMC (RRRMC.jl:81-127) on a stand-alone perceptron.  E = None: a fresh call (E = energy(X, C))"""
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
