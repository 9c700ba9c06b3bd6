"""Plain-Python restatement of the reference's random K-SAT graph, written from src/graphs/SAT.jl (line numbers below are theirs).
``ClauseCache`` keeps the literal S / I / lfields bookkeeping of energy and update_cache!, member order of I included; ``pure_delta`` and
``pure_energy`` are what the engine computes instead (csrc/sat_core.hpp): functions of the configuration alone.  Indices are 0-based
(an empty slot of I is -1 where the reference writes 0).

A ``SatRef`` is usable as a slice class by ``re_reference`` and ``le_reference`` (energy, delta, flip_update): ``re_ensemble`` /
``le_ensemble`` build their ensembles over GraphEmpty and put M copies of one instance in its place, as ``Gconstr(args...)`` with
``X.N, X.A, X.J`` does (src/REAliases.jl:77-92, src/LEAliases.jl:77-92).  Configurations are 0/1 integer arrays (1 = +1)."""
import numpy as np

import le_reference as LE
import re_reference as RE

TAG_GRAPH, TAG_COUPLING = 4, 5          # oracle/philox_contract.h


class ClauseCache:
    """GraphSAT with its ClauseCache and LocalFields (:58-115, :189-320)"""

    def __init__(self, N, A, J):
        self.N, self.A, self.J = N, [list(a) for a in A], [list(j) for j in J]
        self.M = len(A)
        self.K = max(len(a) for a in A)                                # :90
        self.T = [[] for _ in range(N)]                                # :92-97
        for a, Aa in enumerate(self.A):
            for i in Aa:
                self.T[i].append(a)
        self.neighb = [[] for _ in range(N)]                           # :99-107
        for i in range(N):
            for a in self.T[i]:
                for j in self.A[a]:
                    if j != i and j not in self.neighb[i]:
                        self.neighb[i].append(j)
        self.max_conn = max(len(t) for t in self.T)                    # :110
        self.S = [0] * self.M
        self.I = [[-1] * len(a) for a in self.A]
        self.lfields = [0] * N

    def energy(self, s):                                               # :189-231
        self.S = [0] * self.M                                          # clear!
        self.I = [[-1] * len(a) for a in self.A]
        n = 0
        for a in range(self.M):
            sat = 0
            for k, i in enumerate(self.A[a]):
                if self.J[a][k] ^ int(s[i]) == 0:
                    self.I[a][sat] = i
                    sat += 1
            self.S[a] = sat
            n += sat == 0
        for i in range(self.N):
            D = 0
            for a in self.T[i]:
                if self.S[a] == 1 and self.I[a][0] == i:
                    D += 1
                elif self.S[a] == 0:
                    D -= 1
            self.lfields[i] = -D
        return n

    def delta_energy(self, move):                                      # :233-241
        return -self.lfields[move]

    def neighbors(self, i):                                            # :322
        return self.neighb[i]

    def update_cache(self, move):                                      # :258-320, after the flip of s[move]
        S, I, lf = self.S, self.I, self.lfields
        for a in self.T[move]:
            Sa, Ia, Aa = S[a], I[a], self.A[a]
            if Sa == 0:
                S[a] = 1
                Ia[0] = move
                lf[move] -= 2
                for j in Aa:
                    if j != move:
                        lf[j] -= 1
            elif move in Ia:
                k = Ia.index(move)
                for l in range(k, Sa - 1):
                    Ia[l] = Ia[l + 1]
                Ia[Sa - 1] = -1
                S[a] = Sa - 1
                if Sa == 1:
                    lf[move] += 2
                    for j in Aa:
                        if j != move:
                            lf[j] += 1
                elif Sa == 2:
                    lf[Ia[0]] -= 1
            else:
                if Sa == 1:
                    lf[Ia[0]] += 1
                S[a] = Sa + 1
                Ia[Sa] = move


class SatRef(ClauseCache):
    """the slice interface of re_reference / le_reference"""

    def delta(self, s, i):
        return self.delta_energy(i)

    def flip_update(self, s, i):
        self.update_cache(i)


def pure_energy(A, J, s):
    """the definition: clauses without a true literal"""
    return sum(all(int(s[i]) != j for i, j in zip(Aa, Ja)) for Aa, Ja in zip(A, J))


def pure_delta(A, J, T, s, i):
    """#(clauses i alone satisfies) − #(unsatisfied clauses containing i), from the configuration only"""
    d = 0
    for a in T[i]:
        sat = [v for v, j in zip(A[a], J[a]) if int(s[v]) == j]
        if sat == [i]:
            d += 1
        elif not sat:
            d -= 1
    return d


# ---- the generator (:17-56) on the addressed streams ----------------------------------------------------------------------------
def _stream_u64(oracle, seed, tag, n):
    w = oracle.philox([(n >> 1) & 0xffffffff, (n >> 1) >> 32, 0, tag], [seed & 0xffffffff, seed >> 32])
    h = n & 1
    return (int(w[2 * h]) << 32) | int(w[2 * h + 1])


def round_half_even(x):
    """round(Int, x) as Julia rounds a Float64: ties to even"""
    return int(np.rint(np.float64(x)))


def gen_ksat(oracle, N, K, alpha, seed):
    """gen_randomKSAT with choose (:17-40): draw n = a K + k; 0-based variables out"""
    M = round_half_even(np.float64(alpha) * N)
    A, J = [], []
    for a in range(M):
        out = []
        for k in range(K):                                             # choose: out[k] = rand(1:(N-k+1)), 1-based k
            x = 1 + ((_stream_u64(oracle, seed, TAG_GRAPH, a * K + k) * (N - k)) >> 64)
            for l in range(k):
                if out[l] <= x:
                    x += 1
            out.append(x)
            for l in range(k):
                if out[l] > x:
                    for j in range(k, l, -1):
                        out[j] = out[j - 1]
                    out[l] = x
                    break
        A.append([x - 1 for x in out])
        J.append([_stream_u64(oracle, seed, TAG_COUPLING, a * K + k) >> 63 for k in range(K)])
    return A, J


def ragged_instance():
    """N = 20 and 90 clauses of lengths 1 .. 8: unit clauses, variable 19 in no clause, variable 0 in 70 clauses (two ballot passes)"""
    rng = np.random.default_rng(20261018)
    N, A, J = 20, [], []
    for a in range(90):
        l = 1 + a % 8
        if a < 70:
            Aa = [0] + sorted(rng.choice(np.arange(1, 19), l - 1, replace=False).tolist())
        else:
            Aa = sorted(rng.choice(np.arange(1, 19), l, replace=False).tolist())
        A.append([int(i) for i in Aa])
        J.append([int(j) for j in rng.integers(0, 2, l)])
    return N, A, J


def re_ensemble(N, A, J, M, gamma, beta):
    X = RE.make_ensemble(N, M, gamma, beta, "empty")
    X.X1 = [SatRef(N, A, J) for _ in range(M)]
    return X


def le_ensemble(N, A, J, M, gamma, beta):
    X = LE.make_ensemble(N, M, gamma, beta, "empty")
    X.Xc = SatRef(N, A, J)
    X.X1 = [SatRef(N, A, J) for _ in range(M)]
    return X


def standard_mc(X, s, beta, iters, step, seed, oracle, replica=0, it0=0, E=None):
    """standardMC (RRRMC.jl:81-127) on a stand-alone GraphSAT.  E = None: a fresh call (E = energy(X, C)).  Energies as Float64."""
    if E is None:
        E = X.energy(s)
    Es, accepted = [], 0
    for it in range(1, iters + 1):
        if it % step == 0:
            Es.append(float(E))
        g = it0 + it
        move = oracle.site_of(seed, g, X.N)
        dE = X.delta_energy(move)
        x = -beta * dE
        if not (x >= 0 or oracle.rand53(seed, g, replica) < oracle.det_exp(x)):
            continue
        s[move] ^= 1
        X.update_cache(move)
        E += dE
        accepted += 1
    return Es, E, accepted
