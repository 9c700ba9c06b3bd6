"""Plain-Python restatement of the reference's cross-entropy perceptron, written from src/graphs/PercXEntr.jl (line numbers below are its).
The Stabilities keep the reference's two arrays and their literal swap (Δs / newΔs, :30-47, :127-130); the ξsi / last_move copy of one
pattern column (:138, :173) is an access optimisation and is read straight from ξ here.  Every sum is a sequential Float64 loop in pattern
order, as the reference's are.

A ``PercXEntrRef`` has the slice interface of ``perc_reference.PercStepRef`` (energy, delta, flip_update), so ``add_fields_reference`` and
the ``standard_mc`` loop below drive it with the library's addressed random streams.  Configurations are 0/1 integer arrays (1 = +1)."""
import math

import numpy as np


def loss_table(N, lam):
    """Hs (:65): [log(1 + exp(-2 * λ * Δ / √(N))) for Δ = -N:2:N]"""
    return [math.log(1 + math.exp(((-2.0 * lam) * d) / math.sqrt(N))) for d in range(-N, N + 1, 2)]


def d2i(d, N):
    """Δ2i (:49), 0-based"""
    return (d + N) >> 1


class PercXEntrRef:
    """GraphPercXEntr{λ} (:51-87): ET = Float64.  ``Hs``: the table to use instead of building it from λ (the library's contract is "given
    the same table")"""

    def __init__(self, xi, lam=None, Hs=None):
        xi = np.asarray(xi, np.int64)
        self.P, self.N = xi.shape
        if self.N % 2 == 0:
            raise ValueError("N must be odd, given: %d" % self.N)      # :63
        self.xi = xi
        self.Hs = [float(h) for h in (loss_table(self.N, lam) if Hs is None else Hs)]
        assert len(self.Hs) == self.N + 1
        self._empty()

    def with_lambda(self, lam):                                        # GraphPercXEntr(X, λnew) (:87): the patterns are kept, the cache is new
        return PercXEntrRef(self.xi, lam)

    def _empty(self):                                                  # Stabilities(P) (:36-41), empty! (:89-95)
        self.ds = [0] * self.P
        self.newds = [0] * self.P
        self.last_move = -1
        self.just_delta = False

    def energy(self, s):                                               # :97-119
        E = 0.0
        self._empty()
        s = np.asarray(s)
        for a in range(self.P):
            d = self.N - 2 * int((s ^ self.xi[a]).sum())
            self.ds[a] = d
            E += self.Hs[d2i(d, self.N)]
        return E

    def flip_update(self, s, i):                                       # update_cache! (:121-151), after the flip of s[i]
        if self.just_delta and self.last_move == i:                    # :127-130
            self.ds, self.newds = self.newds, self.ds
            return
        si = 1 - int(s[i])                                             # :137: ~s[move], the bit before the flip
        self.last_move = i
        for a in range(self.P):                                        # :142-146
            xsi = int(self.xi[a, i]) ^ si
            self.ds[a] = self.ds[a] + (4 * xsi - 2)
        self.just_delta = False

    def delta(self, s, i):                                             # delta_energy (:165-193)
        si = int(s[i])
        self.last_move = i
        dE = 0.0
        for a in range(self.P):                                        # :178-186
            xsi = int(self.xi[a, i]) ^ si
            old = self.ds[a]
            new = old + (4 * xsi - 2)
            self.newds[a] = new
            dE += self.Hs[d2i(new, self.N)] - self.Hs[d2i(old, self.N)]
        self.just_delta = True
        return dE

    def step_energy(self):                                             # :205-213
        E = 0
        for a in range(self.P):
            E += self.ds[a] < 0
        return E


def standard_mc(X, s, beta, iters, step, seed, oracle, replica=0, it0=0, E=None, hook=None):
    """standardMC (RRRMC.jl:81-127) on a stand-alone GraphPercXEntr.  E = None: a fresh call (E = energy(X, C)); else continue with the given
    tracked E (and X's live cache)."""
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
        s[move] ^= 1
        X.flip_update(s, move)
        E += dE
        accepted += 1
    return Es, E, accepted
