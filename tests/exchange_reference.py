"""Plain-numpy restatement of the replica exchange between two contexts (include/rrrmc_hip.h: rrrmc_exchange_async): the rule on
the oracle's philox / det_exp, the swap on Config bit rows, and a vectorised reference parallel-tempering loop for the law test.

A helper module: no fixture, no pytest setting.  Nothing here calls the HIP library.
"""
from collections import namedtuple

import numpy as np

TAG_EXCHANGE = 14
_M32 = 0xFFFFFFFF


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def uniform(oracle, seed, rnd, replica):
    """u of global replica `replica` in round `rnd`: 53 bits of words 0 and 1 of the EXCHANGE stream's block"""
    w = oracle.philox([rnd & _M32, (rnd >> 32) & _M32, replica & _M32, TAG_EXCHANGE], [seed & _M32, (seed >> 32) & _M32])
    return float(((int(w[0]) << 32 | int(w[1])) >> 11) * 2.0 ** -53)


def x_of(beta_a, beta_b, Ea, Eb):
    """x = (beta_a - beta_b) * (Ea - Eb): three Float64 roundings"""
    dB = np.float64(beta_a) - np.float64(beta_b)
    dE = np.float64(Ea) - np.float64(Eb)
    return float(dB * dE)


def accept_x(oracle, x, u):
    return bool(x >= 0 or u < oracle.det_exp(x))


def flags(oracle, beta_a, beta_b, Ea, Eb, seed, rnd, replica0=0):
    """the verdict of every replica (bool [R]) for the energies Ea[R], Eb[R] in the model's units"""
    return np.array([accept_x(oracle, x_of(beta_a, beta_b, Ea[r], Eb[r]), uniform(oracle, seed, rnd, replica0 + r)) for r in range(len(Ea))], bool)


def mask_words(fl):
    """the swap mask: bit r & 31 of word r >> 5; the padding bits of the last word stay zero"""
    fl = np.asarray(fl, bool)
    m = np.zeros((len(fl) + 31) // 32, np.uint32)
    for r in np.flatnonzero(fl):
        m[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    return m


def swap_rows(sa, sb, fl):
    """the two Config chunk arrays ([R, nch] uint64) after the exchange: the flagged rows trade places"""
    fl = np.asarray(fl, bool)[:, None]
    return np.where(fl, sb, sa), np.where(fl, sa, sb)


# ---- the parity cases of tests/test_gpu_exchange.py (and their condition, checked on the CPU) --------------------------------------
# graph, R, the two engines' seeds and betas, a short run's length, the exchange's seed and round.  The seeds are chosen so that the flags
# of the last, partial word group hold both values (tests/test_exchange_cpu.py checks it through the oracle's chains).
ParityCase = namedtuple("ParityCase", "id make R seed_a seed_b beta_a beta_b iters xseed rnd")
PARITY_CASES = [
    ParityCase("rrg130-bitsliced", lambda pkg: pkg.GraphRRG(130, 3, seed=41), 70, 1001, 2002, 0.9, 0.6, 390, 77, 3),
    ParityCase("sk65-bytes", lambda pkg: pkg.GraphSK(65, seed=42), 9, 1003, 2004, 0.9, 0.6, 195, 78, (1 << 32) + 5),
    ParityCase("skn33-bytes", lambda pkg: pkg.GraphSKNormal(33, seed=43), 9, 1005, 2006, 1.0, 0.7, 99, 79, 4),
    ParityCase("rrgn130-lanes64", lambda pkg: pkg.GraphRRGNormal(130, 3, seed=44), 70, 1007, 2008, 0.9, 0.6, 390, 80, 5),
    ParityCase("rrglev20-rows", lambda pkg: pkg.GraphRRG(20, 3, (-1.0, 0.0, 1.0), seed=45), 5, 1009, 2010, 1.0, 0.6, 60, 81, 6),
]
PARITY_IDS = [c.id for c in PARITY_CASES]


def tail_replicas(R):
    """the replicas of the last, partial word of the swap mask (32 replicas to a word): the group the parity cases' condition is about"""
    return list(range((R - 1) // 32 * 32, R))


def oracle_energy_after(O, X, seed, beta, iters, r):
    """the energy (model units, Float64) replica r holds after standardMC(beta, iters) from the INIT stream's configuration, through the oracle"""
    name = type(X).__name__
    ch = O.init_config(seed, r, X.N)
    if name == "GraphRRG":
        Es = O.standard_mc_sparse(X.A, X.J.astype(np.int32), beta, iters, iters, seed, ch, replica=r, form="rrg")[0]
    elif name == "GraphRRGLevels":
        Es = X.energy_value(O.standard_mc_lev(X.A, X.J.astype(np.int32), beta, iters, iters, seed, ch, replica=r, mul=X.lev_mul, div=X.lev_div)[0])
    elif name == "GraphRRGNormal":
        Es = O.standard_mc_spf(X.A, X.J, beta, iters, iters, seed, ch, replica=r)[0]
    elif name == "GraphSKNormal":
        Es = O.standard_mc_skn(X.J, beta, iters, iters, seed, ch, replica=r)[0]
    elif name == "GraphSK":
        Es = O.standard_mc_skb(X.J, beta, iters, iters, seed, ch, replica=r)[0]
    else:
        raise NotImplementedError(name)
    return float(np.asarray(Es, np.float64)[-1])


# ---- a reference parallel-tempering loop (the law test only; numpy's generator, not the library's streams) -------------------------
def energy_pm(A, J, s):
    """-(1/2) sum_x sum_k J[x, k] s_x s_A[x, k] for s [..., N] of +-1"""
    return -(s[..., :, None] * J[None, :, :] * s[..., A]).sum(axis=(-1, -2)) // 2


def reference_pt(A, J, betas, R, rounds, iters, rng, flip_sign=False):
    """T = len(betas) temperatures x R ladders of random-site Metropolis on the +-J graph (A, J), `rounds` rounds of `iters` attempts and
    the exchanges of the pairs (t, t + 1), t = round (mod 2), by x = (beta_t - beta_t+1)(E_t - E_t+1), swap iff x >= 0 or u < exp(x).
    `flip_sign`: the rule with the sign of x reversed (the law test's wrong sampler).  Returns the final spins [T, R, N] of +-1."""
    A = np.asarray(A, np.int64)
    J = np.asarray(J, np.int64)
    N, T = A.shape[0], len(betas)
    s = (2 * rng.integers(0, 2, size=(T, R, N)) - 1).astype(np.int64)
    E = np.stack([energy_pm(A, J, s[t]) for t in range(T)])
    rows = np.arange(R)
    for rd in range(rounds):
        for t in range(T):
            for _ in range(iters):
                i = rng.integers(0, N, size=R)
                dE = 2 * s[t, rows, i] * (J[i] * s[t][rows[:, None], A[i]]).sum(axis=1)
                acc = rng.random(R) < np.exp(np.minimum(-betas[t] * dE, 0.0))
                s[t, rows[acc], i[acc]] *= -1
                E[t] += np.where(acc, dE, 0)
        for t in range(rd % 2, T - 1, 2):
            x = (betas[t] - betas[t + 1]) * (E[t] - E[t + 1]).astype(np.float64)
            if flip_sign:
                x = -x
            sw = (x >= 0) | (rng.random(R) < np.exp(np.minimum(x, 0.0)))
            s[t][sw], s[t + 1][sw] = s[t + 1][sw].copy(), s[t][sw].copy()
            E[t][sw], E[t + 1][sw] = E[t + 1][sw].copy(), E[t][sw].copy()
    assert all((E[t] == energy_pm(A, J, s[t])).all() for t in range(T))
    return s


def state_index_pm(s):
    """state index of +-1 spins [R, N] in boltzmann_law's order (site 0 the most significant bit, spin +1 = bit 1)"""
    N = s.shape[1]
    bits = (s > 0).astype(np.int64)
    return (bits << (N - 1 - np.arange(N))[None, :]).sum(axis=1)
