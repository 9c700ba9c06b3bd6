"""Plain-Python restatement of the reference's regular 3-spin graph, written from src/graphs/PSpin3.jl (line numbers below are theirs).
``PSpin3Ref`` keeps the literal ``LocalFields{Int}`` cache — lfields, lfields_last, move_last and the swap undo over the unique
neighbours ``U`` — of energy and update_cache!; ``pure_delta`` and ``pure_energy`` are what the engine computes instead
(csrc/pspin_core.hpp): functions of the configuration alone.  Indices are 0-based (move_last = -1 where the reference writes 0).
Configurations are 0/1 integer arrays (1 = +1)."""
import numpy as np


def table_from_triples(N, layers):
    """A [N][2K] of the constructor (:32-43) from explicit layers: layers[k] lists the N / 3 triples (v1, v2, v3) of layer k"""
    K = len(layers)
    A = np.zeros((N, 2 * K), np.int64)
    for k, layer in enumerate(layers):
        for v1, v2, v3 in layer:
            A[v1, 2 * k], A[v1, 2 * k + 1] = v2, v3
            A[v2, 2 * k], A[v2, 2 * k + 1] = v1, v3
            A[v3, 2 * k], A[v3, 2 * k + 1] = v1, v2
    return A


def layers_of(A):
    """the K partitions a table describes, every triple as a sorted tuple; raises where a layer is no partition"""
    A = np.asarray(A)
    N, K = A.shape[0], A.shape[1] // 2
    out = []
    for k in range(K):
        tr = {tuple(sorted((i, int(A[i, 2 * k]), int(A[i, 2 * k + 1])))) for i in range(N)}
        assert len(tr) == N // 3 and sorted(v for t in tr for v in t) == list(range(N)), "layer %d is not a partition" % k
        out.append(tr)
    return out


class PSpin3Ref:
    """GraphPSpin3 with its LocalFields{Int} (:14-53, :62-155)"""

    def __init__(self, N, A):
        A = np.asarray(A)
        assert N % 3 == 0 and A.shape[0] == N and A.shape[1] % 2 == 0                       # :24
        self.N, self.K = N, A.shape[1] // 2
        self.A = [[int(x) for x in a] for a in A]
        self.U = [list(dict.fromkeys(a)) for a in self.A]                                   # unique(a), first occurrences in order: :47
        self.lfields = [0] * N
        self.lfields_last = [0] * N
        self.move_last = -1

    def energy(self, s):                                                                    # :62-93
        n = 0
        for x in range(self.N):
            sx = 2 * int(s[x]) - 1
            Ax = self.A[x]
            lf = 0
            for k in range(self.K):
                sy = 2 * int(s[Ax[2 * k]]) - 1
                sz = 2 * int(s[Ax[2 * k + 1]]) - 1
                lf -= sy * sz
            lf *= sx
            n += lf
            self.lfields[x] = 2 * lf
        assert n % 3 == 0                                                                   # :88
        n //= 3
        self.move_last = -1
        self.lfields_last = [0] * self.N
        return n

    def delta_energy(self, move):                                                           # :147-155
        return -self.lfields[move]

    def neighbors(self, i):                                                                 # :177
        return self.U[i]

    def update_cache(self, s, move):                                                        # :95-145, after the flip of s[move]
        lf, lfl = self.lfields, self.lfields_last
        if self.move_last == move:
            for y in self.U[move]:
                lf[y], lfl[y] = lfl[y], lf[y]
            lf[move] = -lf[move]
            lfl[move] = -lfl[move]
            return
        for y in self.U[move]:
            lfl[y] = lf[y]
        sx = 2 * int(s[move]) - 1
        Ax = self.A[move]
        for k in range(self.K):
            y, z = Ax[2 * k], Ax[2 * k + 1]
            sy = 2 * int(s[y]) - 1
            sz = 2 * int(s[z]) - 1
            D = 4 * sx * sy * sz
            lf[y] -= D
            lf[z] -= D
        lfm = lf[move]
        lfl[move] = lfm
        lf[move] = -lfm
        self.move_last = move

    # the slice interface of add_fields_reference
    def delta(self, s, i):
        return self.delta_energy(i)

    def flip_update(self, s, i):
        self.update_cache(s, i)


def all_delta_e(K):
    """allΔE(GraphPSpin3{K}) (:178-180)"""
    if K % 2 == 0:
        return tuple(4 * (d - 1) for d in range(1, K // 2 + 2))
    return tuple(2 * (2 * d - 1) for d in range(1, (K + 1) // 2 + 1))


def pure_energy(A, s):
    """the definition: −Σ_triples σσσ, every layer's triples taken once"""
    A = np.asarray(A)
    N, K = A.shape[0], A.shape[1] // 2
    sg = 2 * np.asarray(s, np.int64) - 1
    E = 0
    for k in range(K):
        for t in {tuple(sorted((i, int(A[i, 2 * k]), int(A[i, 2 * k + 1])))) for i in range(N)}:
            E -= int(sg[t[0]] * sg[t[1]] * sg[t[2]])
    return E


def pure_delta(A, s, i):
    """2 (2c − K), c = the layers with s_i ⊻ s_y ⊻ s_z == 1, from the configuration only"""
    a = np.asarray(A)[i]
    K = len(a) // 2
    c = sum(int(s[i]) ^ int(s[a[2 * k]]) ^ int(s[a[2 * k + 1]]) for k in range(K))
    return 2 * (2 * c - K)


def standard_mc(X, s, beta, iters, step, seed, oracle, replica=0, it0=0, E=None):
    """standardMC (RRRMC.jl:81-127) on a stand-alone GraphPSpin3.  E = None: a fresh call (E = energy(X, C)).  Energies as Float64."""
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
        X.update_cache(s, move)
        E += dE
        accepted += 1
    return Es, E, accepted
