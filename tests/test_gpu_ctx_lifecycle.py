"""A context owns its device memory (rrrmc.jl_amd/csrc/dev_mem.hpp): the buffers a sampler allocates at its first call and regrows when a later
call takes more samples, contexts created and destroyed in any order, and a multi-device context that fails half-way.  One context per creator
family, at the smallest shapes the kernels accept.

(a) grow path: on one context a call that takes ONE sample, then the same number of iterations with EIGHT samples — every dev_grow site regrows
a live buffer; on a fresh context with the same seed the first call already takes eight samples (same iterations, a shorter step: sampling does
not touch the chain), so its second call regrows nothing.  The second call's samples, counts and the final configuration must be equal, bit for
bit.  Where the oracle is wired here (GraphRRG standardMC and wtmMC, GraphSKNormal standardMC: the calls of tests/test_gpu_sparse_parity.py,
test_gpu_wtm_parity.py and test_gpu_sk_parity.py) the regrown call is compared with the oracle's instead.
No test reads the free device memory: the machines are shared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20260
BETA, TAU, ITERS = 1.0, 1.3, 64


def families(pkg):
    """name -> (graph, replicas, samplers)"""
    all5 = ("std", "rrr", "bkl", "wtm", "eo")
    return {
        "rrg": (lambda: pkg.GraphRRG(64, 3, seed=SEED), 32, all5),
        "skn": (lambda: pkg.GraphSKNormal(32, seed=SEED), 8, all5),
        "skb": (lambda: pkg.GraphSK(32, seed=SEED), 8, all5),
        "spf": (lambda: pkg.GraphRRGNormal(64, 3, seed=SEED), 64, all5),
        "disc": (lambda: pkg.GraphRRGNormalDiscretized(64, 3, (-1, 0, 1), seed=SEED), 4, all5),
        "lev": (lambda: pkg.GraphRRG(64, 3, LEV=(-1, 0, 1), seed=SEED), 4, all5),
        "quant": (lambda: pkg.GraphQuant(pkg.GraphRRG(16, 3, seed=SEED), 4, 0.5, 2.0), 4, all5),
        "perc": (lambda: pkg.GraphPercStep(21, 5, seed=SEED), 4, ("std",)),
        "comm": (lambda: pkg.GraphCommStep(3, 7, 5, seed=SEED), 4, ("std",)),
        "sat": (lambda: pkg.GraphSAT(32, 3, 4.0, seed=SEED), 4, ("std",)),
        "re": (lambda: pkg.Graph0RE(5, 3, 1.0, 1.0), 4, ("std", "rrr")),
        "le": (lambda: pkg.Graph0LE(5, 3, 1.0, 1.0), 4, ("std", "rrr")),
        "tle": (lambda: pkg.Graph0TLE(5, 3, 1.0, 0.5, 1.0), 4, ("std", "rrr")),
    }


CASES = [(f, s) for f, smps in (("rrg", 5), ("skn", 5), ("skb", 5), ("spf", 5), ("disc", 5), ("lev", 5), ("quant", 5), ("perc", 1), ("comm", 1), ("sat", 1),
                                ("re", 2), ("le", 2), ("tle", 2)) for s in ("std", "rrr", "bkl", "wtm", "eo")[:smps]]


def call(eng, smp, nsamp):
    """One sampler call of ITERS iterations (wtmMC: of global time 8 / N) that takes nsamp samples; its results as a list of arrays."""
    step = ITERS // nsamp
    if smp == "std":
        out = eng.standard_mc(BETA, ITERS, step)
    elif smp == "rrr":
        out = eng.rrr_mc(BETA, ITERS, step)
    elif smp == "bkl":
        out = eng.bkl_mc(BETA, ITERS, step)
    elif smp == "wtm":
        out = eng.wtm_mc(BETA, nsamp, 8.0 / nsamp)
    else:
        Es, Emin, Cmin, itmin = eng.extremal_opt(TAU, ITERS, step)
        out = (Es, Emin, Cmin.s, itmin)
    return [np.array(o) for o in out]


def two_calls(pkg, X, R, smp, first_nsamp):
    with pkg.Engine(X, R) as eng:
        eng.seed(SEED)
        eng.init_spins_random()
        C0 = eng.get_config().s.copy()
        call(eng, smp, first_nsamp)
        second = call(eng, smp, 8)
        return C0, second, eng.get_config().s.copy()


@pytest.mark.parametrize("family,smp", CASES)
def test_a_regrown_sample_buffer_changes_nothing(pkg, oracle, family, smp):
    make, R, samplers = families(pkg)[family]
    assert smp in samplers
    X = make()
    C0, grown, cfg = two_calls(pkg, X, R, smp, 1)
    assert grown[0].shape == (R, 8)
    if (family, smp) == ("rrg", "std"):
        A, J = X.A, X.J.astype(np.int32)
        r1 = oracle.standard_mc_sparse_batch(A, J, BETA, ITERS, ITERS, SEED, C0)
        r2 = oracle.standard_mc_sparse_batch(A, J, BETA, ITERS, ITERS // 8, SEED, r1[1], it0=ITERS)
        assert (grown[0] == r2[0]).all() and (grown[1] == r2[2]).all() and (cfg == r2[1]).all()
    elif (family, smp) == ("rrg", "wtm"):
        J = X.J.astype(np.int32)
        for r in range(R):
            r1 = oracle.wtm_mc_sparse(X.A, J, BETA, 1, 8.0, SEED, C0[r], replica=r)
            r2 = oracle.wtm_mc_sparse(X.A, J, BETA, 8, 1.0, SEED, r1[1], call=1, replica=r)
            assert (grown[0][r] == r2[0]).all() and grown[1][r] == r2[2] and grown[2][r] == r2[3] and (cfg[r] == r2[1]).all()
    elif (family, smp) == ("skn", "std"):
        for r in range(R):
            r1 = oracle.standard_mc_skn(X.J, BETA, ITERS, ITERS, SEED, C0[r], replica=r)
            r2 = oracle.standard_mc_skn(X.J, BETA, ITERS, ITERS // 8, SEED, r1[1], it0=ITERS, replica=r)
            assert (grown[0][r] == r2[0]).all() and grown[1][r] == r2[2] and (cfg[r] == r2[1]).all()
    else:
        C0f, fresh, cfgf = two_calls(pkg, make(), R, smp, 8)
        assert (C0 == C0f).all()
        assert len(grown) == len(fresh)
        for g, f in zip(grown, fresh):
            assert g.shape == f.shape and g.dtype == f.dtype and (g == f).all()
        assert (cfg == cfgf).all()


def use(pkg, family):
    """a new context that has run one sampler call (the family's last sampler: it allocates lazily); the caller closes it"""
    make, R, samplers = families(pkg)[family]
    eng = pkg.Engine(make(), R)
    eng.seed(SEED)
    eng.init_spins_random()
    call(eng, samplers[-1], 8)
    return eng


@pytest.mark.parametrize("family", ["rrg", "skn", "spf", "quant", "sat", "le"])
def test_create_use_destroy_three_times(pkg, family):
    for _ in range(3):
        use(pkg, family).close()          # (every library call inside raises unless it returns RRRMC_OK)


@pytest.mark.parametrize("first,second", [("rrg", "skb"), ("spf", "re"), ("disc", "perc"), ("lev", "comm"), ("quant", "tle")])
@pytest.mark.parametrize("reverse", [False, True])
def test_two_contexts_of_different_families_alive_at_once(pkg, first, second, reverse):
    a = use(pkg, first)
    b = use(pkg, second)
    call(a, families(pkg)[first][2][0], 8)          # a still works beside b
    for eng in ((b, a) if reverse else (a, b)):
        eng.close()
    use(pkg, first).close()


def test_a_multi_device_context_that_fails_half_way(pkg):
    """rrrmc_ctx_create_multi with a valid and an out-of-range device: the first shard's context exists when the second's creator refuses, and
    is destroyed with everything it had allocated.  Code and text are those of the library before the contexts kept a registry of their
    allocations (recorded on an MI355X: 1, "device 99 out of range (0..n-1)" with n the number of visible devices); a fresh context on the
    valid device works afterwards."""
    L = pkg.lib()
    n = L.rrrmc_device_count()
    assert n >= 1
    ctx = C.c_void_p()
    ids = np.array([0, 99], np.int32)
    rc = L.rrrmc_ctx_create_multi(C.byref(ctx), 1, 64, 3, 0, 64, ids, 2, 0)          # RRRMC_MODEL_SPARSE_PM1: GraphRRG(64, 3), 2 x 32 replicas
    msg = L.rrrmc_last_error(None).decode()
    assert (rc, msg) == (1, "device 99 out of range (0..%d)" % (n - 1))
    assert ctx.value is None
    use(pkg, "rrg").close()
