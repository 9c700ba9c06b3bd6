"""Plain-Python restatement of the Robust Ensemble — TEST INFRASTRUCTURE, written from the Julia sources (src/graphs/RE.jl, src/RRRMC.jl:81-127
and :221-290, src/DeltaE.jl:63-295, src/ArraySets.jl, src/graphs/SK.jl, src/graphs/Empty.jl), not from the HIP code.

The reference draws from Julia's global RNG; every draw here comes from the project's addressed streams through the oracle's
exports (``philox``, ``site_of``, ``rand53``, ``det_exp``, ``init_config``, ``gen_sk_binary``, ``gen_sk_gauss``), as ``emulate_sweep.py`` does.
Sites are 0-based: site j is spin i = j // M of replica k = j % M (RE.jl:76-95).  The tables are libm's (``math``), and the class of a site is
the integer |mū| // 2 with the `up` bit decided on the Float64 field (DeltaE.jl:80-86; fk(-x) = -fk(x) exactly, so this is findk)."""
import math

import numpy as np

TAG_RRR = 8
MASK64 = (1 << 64) - 1


# ---- GraphRE{M,γ,β} tables (RE.jl:18-26, 53-56, 90-93) -------------------------------------------------------------------------
def logcoshratio(a, b):
    a = abs(a)
    b = abs(b)
    return a - b + (math.log1p(math.exp(-2 * a)) - math.log1p(math.exp(-2 * b)))


def fk(mub, gamma, beta):
    return logcoshratio(gamma * float(mub + 1), gamma * float(mub - 1)) / beta


def tables(M, gamma, beta):
    """(ΔElist: fk(mū) for mū = -(M-1) .. M-1 step 2, e0: log(2 cosh(γ μ)) / β for μ = -M .. M step 2)"""
    dE = [fk(2 * d - (M - 1), gamma, beta) for d in range(M)]
    e0 = [math.log(2 * math.cosh(gamma * float(2 * d - M))) / beta for d in range(M + 1)]
    return dE, e0


def all_delta_e(M, gamma, beta):
    """allΔE(GraphRE{M,γ,β}) (RE.jl:208-213)"""
    K = M - 1
    return [fk(2 * d, gamma, beta) for d in range(K // 2 + 1)] if K % 2 == 0 else [fk(2 * d + 1, gamma, beta) for d in range((K + 1) // 2)]


# ---- slice graphs -----------------------------------------------------------------------------------------------------------------
class SliceEmpty:
    """GraphEmpty (Empty.jl): energy 0, delta_energy 0, no cache"""

    def __init__(self, Nk):
        self.Nk = Nk

    def energy(self, s):
        return 0

    def delta(self, s, i):
        return 0

    def flip_update(self, s, i):
        pass


class SliceSK:
    """binary GraphSK (SK.jl:28-140) with its integer LocalFields; J as [Nk, ceil(Nk/64)] chunk rows"""

    def __init__(self, Jc, Nk):
        self.Nk = Nk
        self.sN = math.sqrt(Nk)
        bits = np.unpackbits(np.ascontiguousarray(Jc, np.uint64).view(np.uint8), bitorder="little").reshape(Nk, -1)[:, :Nk]
        self.J = bits.astype(np.int64)
        self.lf = np.zeros(Nk, np.int64)
        self.lfl = np.zeros(Nk, np.int64)
        self.move_last = -1

    def energy(self, s):
        N = self.Nk
        n = -2 * int(s.sum())
        for i in range(N):
            sc = int((self.J[i] ^ s).sum())
            si = int(s[i])
            lf = -(2 * si - 1) * (N - 1 - 2 * sc)
            self.lf[i] = 2 * (-lf + 2 * si)
            n += lf
        assert n % 2 == 0
        n //= 2
        self.move_last = -1
        self.lfl[:] = 0
        return n / self.sN

    def delta(self, s, i):
        return int(self.lf[i]) / self.sN

    def flip_update(self, s, i):       # update_cache! after the flip (SK.jl:98-135)
        if self.move_last == i:
            self.lf, self.lfl = self.lfl, self.lf
            return
        si = int(s[i])
        lfm = int(self.lf[i])
        Jsij = (si ^ s ^ self.J[i]).astype(np.int64)
        self.lfl[:] = self.lf
        self.lf[:] = self.lf + 8 * Jsij - 4
        self.lfl[i] = lfm
        self.lf[i] = -lfm
        self.move_last = i


class SliceSKN:
    """GraphSKNormal (SK.jl:181-284) with its Float64 LocalFields"""

    def __init__(self, J):
        self.J = np.asarray(J, np.float64)
        self.Nk = self.J.shape[0]
        self.lf = np.zeros(self.Nk)
        self.lfl = np.zeros(self.Nk)
        self.move_last = -1

    def energy(self, s):
        N = self.Nk
        n = 0.0
        for i in range(N):
            si = int(s[i])
            Ji = self.J[i]
            lf = 0.0
            for j in range(N):
                lf += float(1 - 2 * (si ^ int(s[j]))) * float(Ji[j])
            self.lf[i] = 2 * lf
            n -= lf
        n /= 2
        self.move_last = -1
        self.lfl[:] = 0.0
        return n

    def delta(self, s, i):
        return float(self.lf[i])

    def flip_update(self, s, i):       # update_cache! after the flip (SK.jl:239-276); elementwise, no reduction: numpy is exact here
        if self.move_last == i:
            self.lf, self.lfl = self.lfl, self.lf
            return
        si = int(s[i])
        lfm = float(self.lf[i])
        Jsij = (1 - 2 * (si ^ s)).astype(np.float64) * self.J[i]
        self.lfl[:] = self.lf
        self.lf[:] = self.lf + 4 * Jsij
        self.lfl[i] = lfm
        self.lf[i] = -lfm
        self.move_last = i


def make_slices(kind, Nk, M, J=None):
    """M slices sharing one coupling set (Gconstr(args...) with the same args, RE.jl:228-235)"""
    if kind == "empty":
        return [SliceEmpty(Nk) for _ in range(M)]
    if kind == "sk":
        return [SliceSK(J, Nk) for _ in range(M)]
    return [SliceSKN(J) for _ in range(M)]


# ---- ArraySet and DeltaECache ----------------------------------------------------------------------------------------------------
class ArraySet:
    """ArraySets.jl:19-85, 0-based site ids, positions 1-based as the reference keeps them (0 = absent)"""

    def __init__(self, N):
        self.v = [0] * N
        self.pos = [0] * N
        self.t = 0

    def push(self, i):
        self.t += 1
        self.v[self.t - 1] = i
        self.pos[i] = self.t

    def delete(self, i):
        p = self.pos[i]
        self.v[p - 1] = self.v[self.t - 1]
        self.pos[self.v[p - 1]] = p
        self.pos[i] = 0
        self.t -= 1

    def check(self):
        N = len(self.pos)
        c = 0
        for i in range(N):
            if self.pos[i] == 0:
                continue
            c += 1
            assert 1 <= self.pos[i] <= self.t
            assert self.v[self.pos[i] - 1] == i
        assert c == self.t


# ---- the ensemble ----------------------------------------------------------------------------------------------------------------
class RobustEnsemble:
    """GraphRobustEnsemble{M,γ,β,G} with a configuration s (0/1 per site in ABI order): X0 = GraphRE (μ and LocalFields), X1 = the slices,
    C1 = the slices' configurations"""

    def __init__(self, Nk, M, gamma, beta, kind, J=None):
        self.Nk, self.M, self.gamma, self.beta, self.kind = Nk, M, gamma, beta, kind
        self.N = Nk * M
        self.dElist, self.e0 = tables(M, gamma, beta)
        self.L = (M + 1) // 2
        self.X1 = make_slices(kind, Nk, M, J)
        self.C1 = [np.zeros(Nk, np.int64) for _ in range(M)]
        self.mu = [0] * Nk
        self.lf0 = [0.0] * self.N

    def getk(self, mub):                     # RE.jl:57-63
        return self.dElist[(mub + self.M - 1) >> 1]

    # energy(X0, C) (RE.jl:70-104): μ, then Σ_i −log(2cosh(γ μ_i))/β left to right, then the fields
    def energy0(self, s):
        M, Nk = self.M, self.Nk
        self.mu = [0] * Nk
        for j in range(self.N):
            self.mu[j // M] += 2 * int(s[j]) - 1
        n = 0.0
        for i in range(Nk):
            n -= math.log(2 * math.cosh(self.gamma * self.mu[i])) / self.beta
        for j in range(self.N):
            sj = 2 * int(s[j]) - 1
            self.lf0[j] = float(sj) * self.getk(self.mu[j // M] - sj)
        return n

    def energy(self, s):                     # RE.jl:265-283
        E = self.energy0(s)
        for k in range(self.M):
            self.C1[k][:] = s[k::self.M]
            E += self.X1[k].energy(self.C1[k])
        return E

    def update0(self, s, move):              # update_cache!(X0, C, move) after the flip (RE.jl:112-163): the whole group recomputed
        M = self.M
        sx = 2 * int(s[move]) - 1
        i = move // M
        self.mu[i] += 2 * sx
        for y in range(i * M, i * M + M):
            sy = 2 * int(s[y]) - 1
            self.lf0[y] = float(sy) * self.getk(self.mu[i] - sy)

    def spinflip0(self, s, move):            # spinflip!(X0, C, move)
        s[move] ^= 1
        self.update0(s, move)

    def spinflip(self, s, move):             # spinflip!(X::GraphRobustEnsemble, C, move) (RE.jl:246-253)
        s[move] ^= 1
        k, i = move % self.M, move // self.M
        self.C1[k][i] ^= 1
        self.X1[k].flip_update(self.C1[k], i)
        self.update0(s, move)

    def residual(self, move):                # delta_energy_residual (RE.jl:303-310): not divided by M
        k, i = move % self.M, move // self.M
        return self.X1[k].delta(self.C1[k], i)

    def neighbors0(self, move):              # CavityRange (RE.jl:175-206): the group ascending, the move skipped
        j0 = move - move % self.M
        return [y for y in range(j0, j0 + self.M) if y != move]


class DeltaECache:
    """DeltaE.jl:63-103, 0-based classes a + L up"""

    def __init__(self, X, s, beta_s, det_exp):
        self.X = X
        L = X.L
        self.L = L
        self.ae = all_delta_e(X.M, X.gamma, X.beta)
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
        dE = self.X.lf0[j]
        M = self.X.M
        sj = 2 * int(s[j]) - 1
        a = abs(self.X.mu[j // M] - sj) >> 1          # findk: |fk(mū)| = fk(|mū|) = allΔE[|mū| // 2]
        assert abs(dE) == self.ae[a]
        up = dE > 0 or (dE == 0 and s[j] == 1)
        return a + self.L * up

    def f(self, k):
        return self.ft[k - self.L] if k >= self.L else 1.0

    def check(self, s):                      # check_consistency (DeltaE.jl:120-135) + the classes agree with the configuration
        for a in self.sets:
            a.check()
        for j, k in enumerate(self.pos):
            assert 0 <= k < 2 * self.L
            assert 1 <= self.sets[k].pos[j] <= self.sets[k].t
            for k1 in range(2 * self.L):
                if k1 != k:
                    assert self.sets[k1].pos[j] == 0
            assert k == self.classify(j, s)


# ---- random streams -----------------------------------------------------------------------------------------------
def _u53(w0, w1):
    return float((((int(w0) << 32) | int(w1)) >> 11)) * 2.0 ** -53


def rrr_draws(oracle, seed, g, rep, sub):
    return oracle.philox([g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, rep, TAG_RRR | (sub << 8)], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])


def config_from_chunks(ch, N):
    return np.array([(int(ch[j >> 6]) >> (j & 63)) & 1 for j in range(N)], np.int64)


def chunks_from_config(s):
    N = len(s)
    ch = np.zeros((N + 63) // 64, np.uint64)
    for j in range(N):
        if s[j]:
            ch[j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return ch


# ---- samplers --------------------------------------------------------------------------------------------------------------------
def make_ensemble(Nk, M, gamma, beta, kind, J=None):
    X = RobustEnsemble(Nk, M, gamma, beta, kind, J)
    X._Jc = J                                # the slices' coupling set, for fresh copies
    return X


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
        dE = X.lf0[move] + X.residual(move)
        x = -beta * dE
        if not (x >= 0 or oracle.rand53(seed, g, replica) < oracle.det_exp(x)):
            continue
        X.spinflip(s, move)
        E += dE
        accepted += 1
    return Es, E, accepted


class RrrRun:
    """rrrMC(X::DoubleGraph) (RRRMC.jl:221-290) as a resumable chain: __init__ is the call's start (energy + gen_ΔEcache), run(n) the loop"""

    def __init__(self, X, s, beta, seed, oracle, replica=0, it0=0, staged_thr=0.5, staged_thr_fact=5.0, check_E=False):
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
        self.check_E = check_E

    def _uniform_accept(self, c, x, g):
        if c >= 1 and x >= 0:
            return True
        a = c * self.O.det_exp(x)
        if a >= 1:
            return True
        w = rrr_draws(self.O, self.seed, g, self.rep, 1)
        return _u53(w[0], w[1]) < a

    def run(self, n, step, hook=None):
        X, s, C = self.X, self.s, self.cache
        L = C.L
        Es = []
        for _ in range(n):
            self.it += 1
            it = self.it
            if it % step == 0:
                Es.append(self.E)
                if hook is not None and not hook(it, s, self.accepted, self.E):
                    break
            g = self.g0 + it
            w = rrr_draws(self.O, self.seed, g, self.rep, 0)
            # rand_move (DeltaE.jl:146-167)
            r = _u53(w[0], w[1]) * C.z
            cT = 0.0
            k = 0
            for k in range(2 * L):
                cT += C.T[k]
                if r < cT:
                    break
            if not r < cT:
                while C.T[k] == 0:
                    k -= 1
            dE0 = -C.ae[k] if k < L else C.ae[k - L]
            u = (int(w[2]) << 32) | int(w[3])
            move = C.sets[k].v[(u * C.sets[k].t) >> 64]
            acc = False
            if self.acc_rate < self.staged_thr:
                self.staged_its += 1
                # compute_staged! (DeltaE.jl:202-230) on X0 only, then compute_reverse_probabilities!
                X.spinflip0(s, move)
                staged = []
                for j in X.neighbors0(move):
                    k0 = C.pos[j]
                    k1 = C.classify(j, s)
                    if k0 != k1:
                        staged.append((j, k0, k1))
                k0 = C.pos[move]
                staged.append((move, k0, k0 - L if k0 >= L else k0 + L))
                X.spinflip0(s, move)
                Tp, zp = list(C.T), C.z
                for (_, k0, k1) in staged:
                    f0, f1 = C.f(k0), C.f(k1)
                    Tp[k0] -= f0
                    Tp[k1] += f1
                    zp += f1 - f0
                c = C.z / zp
                dE1 = X.residual(move)
                if self._uniform_accept(c, -self.beta * dE1, g):
                    X.spinflip(s, move)
                    for (j, k0, k1) in staged:           # apply_staged!
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
                if self._uniform_accept(c, -self.beta * dE1, g):
                    self.E += dE0 + dE1
                    self.accepted += 1
                    acc = True
                else:
                    self.apply_move(move)
            self.acc_rate = self.acc_rate * (1 - self.lam) + (1.0 if acc else 0.0) * self.lam
            if self.check_E:                 # the reference's own check (RRRMC.jl:250), on a fresh graph object
                assert abs(self.E - energy_fresh(X.Nk, X.M, X.gamma, X.beta, X.kind, X._Jc, s)) < 1e-10
        return Es

    def apply_move(self, move):              # DeltaE.jl:232-295
        X, s, C = self.X, self.s, self.cache
        L = C.L
        X.spinflip(s, move)
        zp = C.z
        for j in X.neighbors0(move):
            k0 = C.pos[j]
            k1 = C.classify(j, s)
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
        k1 = k0 - L if k0 >= L else k0 + L
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
        """(pos[N], sizes[2L]) as rrrmc_rrr_cache returns them"""
        return np.array(self.cache.pos, np.int8), np.array([a.t for a in self.cache.sets], np.int32)


def energy_fresh(Nk, M, gamma, beta, kind, J, s):
    """energy(X, C) of a fresh graph object (does not disturb a running one)"""
    return make_ensemble(Nk, M, gamma, beta, kind, J).energy(np.array(s, np.int64))


def re_energies(Nk, M, kind, J, s):
    """REenergies of configuration s (a fresh slice per replica)"""
    out = []
    for k in range(M):
        sl = np.asarray(s[k::M], np.int64)
        X1 = make_slices(kind, Nk, 1, J)[0]
        out.append(float(X1.energy(sl)))
    return out
