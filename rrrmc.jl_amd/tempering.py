"""Parallel tempering over a ladder of inverse temperatures: one ``Engine`` (one device context) per β, all of one graph object, and
``Engine.exchange`` between neighbours.  R independent ladders run side by side: ladder r is replica r of every context."""
import numpy as np

from .engine import Engine
from .graphs import DEFAULT_SEED

_M64 = 2 ** 64 - 1


def ladder_seed(seed, t):
    """The seed of the context at temperature index t: splitmix64 of ``seed + (t + 1) * 0x9E3779B97F4A7C15`` (mod 2^64), so that the
    temperatures share neither the SITE nor the ACCEPT nor the INIT stream.  The EXCHANGE stream is keyed by ``seed`` itself."""
    z = (int(seed) + (int(t) + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def check_betas(betas):
    """The ladder as a float64 array; ValueError unless it holds at least two finite, strictly monotone values."""
    try:
        b = np.array([float(x) for x in betas], np.float64)
    except (TypeError, ValueError):
        raise ValueError("betas must be a sequence of numbers")
    if b.size < 2:
        raise ValueError("a ladder needs at least two betas, given %d" % b.size)
    if not np.all(np.isfinite(b)):
        raise ValueError("every beta must be finite, given %r" % (b.tolist(),))
    d = np.diff(b)
    if not (np.all(d > 0) or np.all(d < 0)):
        raise ValueError("betas must be strictly monotone, given %r" % (b.tolist(),))
    return b


class ParallelTempering:
    """``ParallelTempering(X, betas, R=1, device=0, devices=None, seed=DEFAULT_SEED)``: context t holds R replicas of X at betas[t],
    seeded with ``ladder_seed(seed, t)`` and started from random spins.  ``run`` alternates standardMC on every context with exchange
    attempts between neighbouring temperatures; everything is queued on the device, and the host waits once per round for the flags."""

    def __init__(self, X, betas, R=1, device=0, devices=None, seed=DEFAULT_SEED):
        self.betas = check_betas(betas)
        if int(R) < 1:
            raise ValueError("R must be >= 1, given %r" % (R,))
        self.X, self.R, self.T, self.seed = X, int(R), int(self.betas.size), int(seed) & _M64
        self._engines = []
        try:
            for t in range(self.T):
                e = Engine(X, self.R, device=device, devices=devices)
                self._engines.append(e)
                e.seed(ladder_seed(self.seed, t))
                e.init_spins_random()
        except Exception:
            self.close()
            raise
        self.round = 0                                                    # exchange rounds made so far (the EXCHANGE stream's round)
        self.labels = np.repeat(np.arange(self.T)[:, None], self.R, axis=1)   # [T][R] start temperature of the walker now at t
        self.round_trips = np.zeros(self.R, np.int64)
        self.energies = []                                                # per round: [T][R] energies after the round's sampling, before its swaps
        self.swaps = []                                                   # per round: [T - 1][R] bool, pair (t, t + 1) swapped in ladder r
        self.attempted = []                                               # per round: [T - 1] bool, pair (t, t + 1) was tried
        self._acc = np.zeros(self.T - 1, np.int64)
        self._att = np.zeros(self.T - 1, np.int64)
        self._phase = np.zeros((self.T, self.R), np.int8)                 # per walker (by start temperature): 1 after the bottom, 2 after the top
        self._phase[0, :] = 1

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        for e in getattr(self, "_engines", []):
            e.close()
        self._engines = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- access -----------------------------------------------------------------------------------
    def engine(self, t):
        return self._engines[t]

    def config(self, t):
        return self._engines[t].get_config()

    def overlap_hist(self, t):
        """P(q) at betas[t] as a histogram over the R replicas' pairs: ``overlap_moments(pt.overlap_hist(t), N)``."""
        return self._engines[t].overlap_hist(-1, -1)

    @property
    def accept_rate(self):
        """[T - 1]: accepted / attempted exchanges of the pair (t, t + 1) over all rounds and ladders (nan before its first attempt)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self._att > 0, self._acc / np.maximum(self._att, 1), np.nan)

    # -- the run ----------------------------------------------------------------------------------
    def run(self, rounds, iters, step=None, hook=None):
        """``rounds`` rounds of: ``standard_mc_async(betas[t], iters, step)`` on every context (step = iters by default: one sample, taken
        like the reference's before the move of iteration ``iters``), then the exchanges of the pairs (t, t + 1) with t ≡ round (mod 2)
        in ascending t, then ``hook(round, pt)`` if given (a ``False`` from it stops the run).  Returns the number of rounds made."""
        iters = int(iters)
        step = max(iters, 1) if step is None else int(step)
        done = 0
        for _ in range(int(rounds)):
            rd = self.round
            for t, e in enumerate(self._engines):
                e.standard_mc_async(self.betas[t], iters, step)
            pairs = list(range(rd % 2, self.T - 1, 2))
            for t in pairs:
                self._engines[t].exchange(self._engines[t + 1], self.betas[t], self.betas[t + 1], self.seed, rd, wait=False)
            E = np.full((self.T, self.R), np.nan)
            sw = np.zeros((self.T - 1, self.R), bool)
            att = np.zeros(self.T - 1, bool)
            for t in pairs:
                sw[t], E[t], E[t + 1] = self._engines[t].exchange_results()
                att[t] = True
            paired = set(pairs) | {t + 1 for t in pairs}
            for t in range(self.T):                                       # a temperature without a partner this round: the energy its
                if t not in paired:                                       # sampler tracked (a copy of the tracked values, no energy pass)
                    E[t] = self._engines[t].run_energy()
            self._record(sw, att, E)
            self.round += 1
            done += 1
            if hook is not None and hook(rd, self) is False:
                break
        return done

    def _record(self, sw, att, E):
        for t in np.flatnonzero(att):
            s = sw[t]
            lo, hi = self.labels[t].copy(), self.labels[t + 1].copy()
            self.labels[t] = np.where(s, hi, lo)
            self.labels[t + 1] = np.where(s, lo, hi)
            self._acc[t] += int(s.sum())
            self._att[t] += self.R
        r = np.arange(self.R)
        top, bot = self.labels[self.T - 1], self.labels[0]                # the walkers now at the two ends
        up = self._phase[top, r] == 1
        self._phase[top[up], r[up]] = 2
        back = self._phase[bot, r] == 2
        self.round_trips[r[back]] += 1
        self._phase[bot, r] = 1
        self.energies.append(E)
        self.swaps.append(sw)
        self.attempted.append(att)
