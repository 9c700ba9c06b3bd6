"""GraphQuant over pattern-machine slices — GraphQPercStepT, GraphQPercLinearT, GraphQCommStepT, GraphQCommReLUT (src/QAliases.jl:85-159) —
restated literally from the Julia sources, sharing no code with the kernels: GraphQT (src/graphs/QT.jl:42-122), GraphQuant's energy / residual /
spinflip! (:172-199, 270-286), DeltaECache{Float64,2} over GraphQT (src/DeltaE.jl:63-295), rrrMC(X::DoubleGraph) (src/RRRMC.jl:221-290) and
standardMC (:81-127).  The slices are the objects of tests/perc_reference.py and tests/comm_reference.py (or any object with energy / delta /
flip_update).  0-based sites x = k Nk + i.  Draws: the oracle's philox / site_of / rand53 / det_exp on the streams of DESIGN.md §2."""
import math

import numpy as np

from re_reference import ArraySet, _u53, rrr_draws


class GraphQT:
    """GraphQT{fourK} (QT.jl:42-111)"""

    def __init__(self, N, M, fourK):
        if M <= 2:
            raise ValueError("M must be greater than 2, given: %d" % M)          # :47
        assert N % M == 0
        self.N, self.M, self.Nk, self.fourK = N, M, N // M, fourK

    def energy0(self, s):                        # :68-82
        M, Nk = self.M, self.Nk
        n = 0
        for i in range(Nk):
            sj = int(s[i + (M - 1) * Nk])
            for k in range(M):
                sk = int(s[i + k * Nk])
                n -= 1 - 2 * (sk ^ sj)
                sj = sk
        return n

    def energy(self, s):                         # :84
        return self.energy0(s) * self.fourK / 4

    def neighbors(self, i):                      # :105-108
        N, Nk = self.N, self.Nk
        return (i - Nk + (N if i < Nk else 0), i + Nk - (N if i + Nk >= N else 0))

    def delta(self, s, move):                    # :86-103
        k1, k2 = self.neighbors(move)
        sk, s1, s2 = int(s[move]), int(s[k1]), int(s[k2])
        d = (sk ^ (1 - s1)) - (sk ^ s2)
        return d * self.fourK

    def all_delta_e(self):                       # :111
        return (0.0, self.fourK)


class SliceZero:
    """a slice graph of zero energy (GraphEmpty): the Trotter part alone"""

    def energy(self, s):
        return 0

    def delta(self, s, i):
        return 0

    def flip_update(self, s, i):
        pass


def quant_fourK(beta, Gamma, M):                 # QT.jl:165
    return round(2.0 / beta * math.log(1.0 / math.tanh(beta * Gamma / M)), 8)


class GraphQuantRef:
    """GraphQuant{fourK,G} (QT.jl:126-286) over the given slice objects"""

    def __init__(self, Nk, M, fourK, slices):
        assert len(slices) == M
        self.N, self.M, self.Nk = Nk * M, M, Nk
        self.X0 = GraphQT(Nk * M, M, fourK)
        self.X1 = slices
        self.C1 = [np.zeros(Nk, np.int64) for _ in range(M)]

    def energy(self, s):                         # :185-199
        E = self.X0.energy(s)
        for k in range(self.M):
            self.C1[k][:] = s[k * self.Nk:(k + 1) * self.Nk]
            E += self.X1[k].energy(self.C1[k]) / self.M
        return E

    def renergies(self):                         # :201-211
        return [self.X1[k].energy(self.C1[k]) for k in range(self.M)]

    def residual(self, move):                    # :270-281
        k, i = divmod(move, self.Nk)
        return self.X1[k].delta(self.C1[k], i) / self.M

    def delta(self, s, move):                    # :283-286
        return self.X0.delta(s, move) + self.residual(move)

    def spinflip0(self, s, move):                # spinflip!(X0, C, move): GraphQT has no cache
        s[move] ^= 1

    def spinflip(self, s, move):                 # spinflip!(X, C, move) (Interface.jl) + update_cache! (:172-183)
        s[move] ^= 1
        k, i = divmod(move, self.Nk)
        self.C1[k][i] ^= 1
        self.X1[k].flip_update(self.C1[k], i)


class DeltaECacheQT:
    """DeltaECache{Float64,2} over X0 = GraphQT (DeltaE.jl:63-103); 0-based classes a + 2 up"""
    L = 2

    def __init__(self, X0, s, beta, det_exp):
        self.X0 = X0
        self.ae = X0.all_delta_e()
        self.sets = [ArraySet(X0.N) for _ in range(4)]
        self.pos = [0] * X0.N
        for j in range(X0.N):
            self.pos[j] = self.classify(j, s)
            self.sets[self.pos[j]].push(j)
        self.ft = [det_exp(-beta * dE) for dE in self.ae]
        self.T = [0.0] * 4
        self.z = 0.0
        for k in range(4):
            x = self.sets[k].t * self.f(k)
            self.z += x
            self.T[k] = x

    def classify(self, j, s):                    # :80-86
        dE = self.X0.delta(s, j)
        a = self.ae.index(abs(dE))
        up = dE > 0 or (dE == 0 and s[j] == 1)
        return a + 2 * up

    def f(self, k):                              # get_class_f
        return self.ft[k - 2] if k >= 2 else 1.0

    def check(self, s):                          # check_consistency (:120-135), and the classes agree with the configuration
        for a in self.sets:
            a.check()
        for j, k in enumerate(self.pos):
            assert 0 <= k < 4 and 1 <= self.sets[k].pos[j] <= self.sets[k].t
            assert all(self.sets[k1].pos[j] == 0 for k1 in range(4) if k1 != k)
            assert k == self.classify(j, s)
        assert sum(a.t for a in self.sets) == self.X0.N


def standard_mc(X, s, beta, iters, step, seed, oracle, replica=0, it0=0, E=None):
    """standardMC (RRRMC.jl:81-127).  E = None: a fresh call (E = energy(X, C)); else continue with the given tracked E."""
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
        X.spinflip(s, move)
        E += dE
        accepted += 1
    return Es, E, accepted


class RrrRun:
    """rrrMC(X::DoubleGraph) (RRRMC.jl:221-290) as a resumable chain: __init__ is the call's start (energy + gen_ΔEcache, :237-240), run(n) the
    loop.  `classes` records the class drawn at every iteration, `branches` whether it was staged and whether it was accepted."""

    def __init__(self, X, s, beta, seed, oracle, replica=0, it0=0, staged_thr=0.5, staged_thr_fact=5.0, fresh_energy=None):
        self.X, self.s, self.beta, self.seed, self.O, self.rep = X, s, beta, seed, oracle, replica
        self.E = X.energy(s)
        self.cache = DeltaECacheQT(X.X0, s, beta, oracle.det_exp)
        self.lam = staged_thr_fact / X.N         # :243
        self.staged_thr = staged_thr
        self.acc_rate = 0.5
        self.it, self.g0 = 0, it0
        self.accepted = self.staged_its = 0
        self.fresh_energy = fresh_energy         # s -> energy(X, C) on a fresh graph object: the reference's check (:250) after every iteration
        self.classes, self.branches = [], []

    def _accept(self, c, x, g):                  # RRRMC.jl:40-44
        if c >= 1 and x >= 0:
            return True
        a = c * self.O.det_exp(x)
        if a >= 1:
            return True
        w = rrr_draws(self.O, self.seed, g, self.rep, 1)
        return _u53(w[0], w[1]) < a

    def run(self, n, step):
        X, s, C = self.X, self.s, self.cache
        Es = []
        for _ in range(n):
            self.it += 1
            if self.it % step == 0:
                Es.append(self.E)
            g = self.g0 + self.it
            w = rrr_draws(self.O, self.seed, g, self.rep, 0)
            r = _u53(w[0], w[1]) * C.z           # rand_move (DeltaE.jl:146-167)
            cT, k = 0.0, 0
            for k in range(4):
                cT += C.T[k]
                if r < cT:
                    break
            if not r < cT:
                while C.T[k] == 0:
                    k -= 1
            dE0 = -C.ae[k] if k < 2 else C.ae[k - 2]
            u = (int(w[2]) << 32) | int(w[3])
            move = C.sets[k].v[(u * C.sets[k].t) >> 64]
            self.classes.append(k)
            acc = False
            staged_branch = self.acc_rate < self.staged_thr
            if staged_branch:                    # step_rrr (RRRMC.jl:131-138): compute_staged! on X0 (DeltaE.jl:202-230) + reverse probabilities
                self.staged_its += 1
                X.spinflip0(s, move)
                staged = []
                for j in X.X0.neighbors(move):
                    k0, k1 = C.pos[j], C.classify(j, s)
                    if k0 != k1:
                        staged.append((j, k0, k1))
                k0 = C.pos[move]
                staged.append((move, k0, k0 - 2 if k0 >= 2 else k0 + 2))
                X.spinflip0(s, move)
                Tp, zp = list(C.T), C.z
                for (_, k0, k1) in staged:
                    f0, f1 = C.f(k0), C.f(k1)
                    Tp[k0] -= f0
                    Tp[k1] += f1
                    zp += f1 - f0
                c = C.z / zp
                dE1 = X.residual(move)
                if self._accept(c, -self.beta * dE1, g):
                    X.spinflip(s, move)
                    for (j, k0, k1) in staged:   # apply_staged!
                        C.sets[k0].delete(j)
                        C.sets[k1].push(j)
                        C.pos[j] = k1
                    C.T, C.z = Tp, zp
                    self.E += dE0 + dE1
                    self.accepted += 1
                    acc = True
            else:
                dE1 = X.residual(move)
                c = self.apply_move(move)
                if self._accept(c, -self.beta * dE1, g):
                    self.E += dE0 + dE1
                    self.accepted += 1
                    acc = True
                else:
                    self.apply_move(move)
            self.branches.append((staged_branch, acc))
            self.acc_rate = self.acc_rate * (1 - self.lam) + (1.0 if acc else 0.0) * self.lam      # :281
            if self.fresh_energy is not None:
                assert abs(self.E - self.fresh_energy(s)) < 1e-10
        return Es

    def apply_move(self, move):                  # DeltaE.jl:232-295
        X, s, C = self.X, self.s, self.cache
        X.spinflip(s, move)
        zp = C.z
        for j in X.X0.neighbors(move):
            k0, k1 = C.pos[j], C.classify(j, s)
            if k0 == k1:
                continue
            f0, f1 = C.f(k0), C.f(k1)
            C.T[k0] -= f0
            C.T[k1] += f1
            zp += f1 - f0
            C.sets[k0].delete(j)
            C.sets[k1].push(j)
            C.pos[j] = k1
        k0 = C.pos[move]
        k1 = k0 - 2 if k0 >= 2 else k0 + 2
        f0, f1 = C.f(k0), C.f(k1)
        C.T[k0] -= f0
        C.T[k1] += f1
        zp += f1 - f0
        C.sets[k0].delete(move)
        C.sets[k1].push(move)
        C.pos[move] = k1
        c = C.z / zp
        C.z = zp
        return c

    def cache_view(self):
        """(pos[N], sizes[4]) as rrrmc_rrr_cache returns them"""
        return np.array(self.cache.pos, np.int8), np.array([a.t for a in self.cache.sets], np.int32)


# ---- the cases of the GPU parity tests (tests/test_gpu_quant_pattern_parity.py), and their CPU preconditions --------------------------------
# (id, slice kind, shape, M, P, fc).  kind: pstep | plin | cstep | crelu; shape: Nk for the perceptrons, (K1, K2) for the committee machines.
CASES = [
    ("pstep-33-3-65", "pstep", 33, 3, 65, False),         # slices straddle 32-bit spin words; two pattern words with a one-bit tail
    ("plin-33-3-65", "plin", 33, 3, 65, False),
    ("pstep-min-3-3-1", "pstep", 3, 3, 1, False),         # the minimum shape
    ("plin-min-3-3-1", "plin", 3, 3, 1, False),
    ("pstep-21-5-64", "pstep", 21, 5, 64, False),         # exactly one full pattern word
    ("plin-21-5-64", "plin", 21, 5, 64, False),
    ("cstep-3x3-3-65", "cstep", (3, 3), 3, 65, False),
    ("cstep-3x3-3-65-fc", "cstep", (3, 3), 3, 65, True),
    ("crelu-2x2-3-65", "crelu", (2, 2), 3, 65, False),
    ("crelu-4x2-3-65", "crelu", (4, 2), 3, 65, False),
    ("crelu-4x2-3-65-fc", "crelu", (4, 2), 3, 65, True),
]
CASE_IDS = [c[0] for c in CASES]
GAMMA, BETA_GRAPH = 0.6, 2.0                     # Γ and the β of fourK
SEED, ITERS, STEP = 0xABCD, 600, 50
# the sampler's β per slice family: the training errors of PercStep / Comm slices are integers / M, PercLinear's are in units of 2 / √Nk
BETA = {"pstep": 1.5, "plin": 2.0, "cstep": 1.5, "crelu": 1.5}
STAGED_THR = 0.55                                # around the run's acceptance rate, so that it crosses between the two branches


def make_graph(pkg, case):
    """the product package's graph of a case"""
    _, kind, shape, M, P, fc = case
    if kind == "pstep":
        return pkg.GraphQPercStepT(shape, P, M, GAMMA, BETA_GRAPH, seed=17)
    if kind == "plin":
        return pkg.GraphQPercLinearT(shape, P, M, GAMMA, BETA_GRAPH, seed=17)
    G = pkg.GraphQCommStepT if kind == "cstep" else pkg.GraphQCommReLUT
    return G(shape[0], shape[1], P, M, GAMMA, BETA_GRAPH, fc=fc, seed=17)


def make_reference(X):
    """the reference object of a product graph: its slices from the public pattern arrays"""
    import comm_reference as CR
    import perc_reference as PR
    X1 = X.X1
    xi = X1.patterns()
    name = type(X1).__name__
    if name in ("GraphPercStep", "GraphPercLinear"):
        mk = lambda: PR.make(xi, name == "GraphPercLinear")
    else:
        mk = lambda: CR.make(X1.K2, xi, X1.labels())
    return GraphQuantRef(X.Nk, X.M, X.fourK, [mk() for _ in range(X.M)])
