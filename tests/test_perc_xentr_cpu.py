"""GraphPercXEntr without a GPU: the plain-Python restatement (tests/xentr_reference.py) held to the reference's own check_delta and to
stabilities from scratch, the front end's loss table against the formula, what the creators refuse before any device is asked for, the
header / _lib.py / Julia contact surface, and the exact Boltzmann law on the restatement alone at the settings the GPU twin
(tests/test_gpu_perc_xentr_boltzmann.py) holds the library to."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import boltzmann_law as BL
import xentr_reference as XR
from test_julia_binding import header_signatures, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERC_XENTR = 11          # RRRMC_RE_SLICE_PERC_XENTR


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,lam", [(5, 3, 1.0), (33, 70, 0.7), (129, 130, 6.0)])
def test_delta_is_the_energy_difference_and_the_cache_follows_a_walk(N, P, lam):
    """check_delta (PercXEntr.jl:195-203): |energy(flipped) − energy − delta| <= atol = 1e-9 along a random walk; Δs kept by flip_update (the
    swap path after a delta of the same move, the loop otherwise) equal Δs from scratch"""
    rng = np.random.default_rng(N)
    xi = rng.integers(0, 2, (P, N))
    X, s = XR.PercXEntrRef(xi, lam), rng.integers(0, 2, N).astype(np.int64)
    X.energy(s)
    for t in range(300):
        i = int(rng.integers(N))
        d = X.delta(s, i)
        fresh = XR.PercXEntrRef(xi, lam)
        e0 = fresh.energy(s)
        s2 = s.copy()
        s2[i] ^= 1
        e1 = fresh.energy(s2)
        assert abs((e1 - e0) - d) <= 1e-9, (t, e1, e0, d)
        if t % 3 == 0:
            continue                                                   # a rejected move: the next delta overwrites newΔs
        if t % 3 == 1:
            i = int(rng.integers(N))                                   # a flip with no delta of the same move before it: the loop path
            X.just_delta = X.just_delta and X.last_move == i
        s[i] ^= 1
        X.flip_update(s, i)
        scratch = XR.PercXEntrRef(xi, lam)
        scratch.energy(s)
        assert X.ds == scratch.ds, t
        assert X.step_energy() == sum(dd < 0 for dd in scratch.ds)


def test_the_front_end_builds_the_table_of_the_formula(pkg):
    for N, lam in ((5, 1.0), (33, 0.3), (129, 6.0), (1001, 2.5)):
        X = pkg.GraphPercXEntr(N, 4, lam, seed=3)
        want = [math.log(1 + math.exp(((-2.0 * lam) * d) / math.sqrt(N))) for d in range(-N, N + 1, 2)]
        assert X.Hs.dtype == np.float64 and X.Hs.tolist() == want and X.Hs.tolist() == XR.loss_table(N, lam)
    X = pkg.GraphPercXEntr(33, 70, 0.7, seed=5)
    Y = pkg.GraphPercXEntr(X, 1.9)                                     # GraphPercXEntr(X, λnew): the patterns stay, the table is λnew's
    assert (Y.xi == X.xi).all() and (Y.N, Y.P, Y.lam) == (33, 70, 1.9) and Y.Hs.tolist() == XR.loss_table(33, 1.9)
    Z = pkg.GraphPercXEntr.from_patterns(X.patterns(), 0.7)
    assert (Z.xi == X.xi).all() and Z.Hs.tolist() == X.Hs.tolist()
    with pytest.raises(ValueError, match="N must be odd"):
        pkg.GraphPercXEntr(32, 4, 1.0)
    with pytest.raises(TypeError, match="Float64"):
        pkg.GraphPercXEntr(33, 4, 1)                                   # PercXEntr.jl:62
    with pytest.raises(ValueError, match="not finite"):
        pkg.GraphPercXEntr(1001, 4, 400.0)                             # exp overflows: the table would hold Inf
    A = pkg.GraphAddSubFields(np.zeros(33), X)
    assert (A.slice_kind, A.model_kind, A._multi_args()) == (11, 101, (101, 33, 0, 0)) and pkg.GraphAddFields(np.zeros(33), X).model_kind == 100
    with pytest.raises(TypeError):
        pkg.GraphRobustEnsemble(33, 3, 1.0, 1.0, X)                    # no RE / LE / Q alias in the reference
    with pytest.raises(TypeError):
        pkg.GraphLocalEntropy(33, 3, 1.0, 1.0, X)


# ---- refusals before any device query -----------------------------------------------------------------------------------------------------
def _call(pkg, name, argtypes, *args):
    lib = pkg.lib()
    ctx = C.c_void_p()
    f = getattr(C.CDLL(lib._name), name)
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_void_p)] + argtypes
    null_out = args[0]
    rc = f(None if null_out else C.byref(ctx), *args[1:])
    msg = lib.rrrmc_last_error(None)
    assert ctx.value is None
    return int(rc), (msg.decode() if msg else "")


def test_the_creators_refuse_by_name_before_any_device_query(pkg):
    I32, I64, U32 = C.c_int32, C.c_int64, C.c_uint32
    xe = lambda null_out=False, N=33, R=4, device=0, replica0=0: _call(pkg, "rrrmc_ctx_create_perc_xentr", [I64, I64, I32, U32], null_out, N, R, device, replica0)
    pc = lambda null_out=False, N=33, R=4, device=0, replica0=0: _call(pkg, "rrrmc_ctx_create_perc", [I64, I32, I64, I32, U32], null_out, N, 1, R, device, replica0)
    af = lambda null_out=False, kind=PERC_XENTR, sub=0, N=33, K2=0, R=4, device=0, replica0=0: _call(
        pkg, "rrrmc_ctx_create_af", [I32, I32, I64, I64, I64, I32, U32], null_out, kind, sub, N, K2, R, device, replica0)
    cases = [(dict(null_out=True), 1, "out is NULL"), (dict(N=0), 1, "N and R must be >= 1"), (dict(R=0), 1, "N and R must be >= 1"),
             (dict(N=20), 1, "N must be odd"), (dict(N=32769), 3, "perceptron kernels"), (dict(N=0, replica0=16), 1, "N and R must be >= 1"),
             (dict(N=20, replica0=16), 1, "N must be odd"), (dict(replica0=16), 1, "replica0 must be a multiple of 32"), (dict(replica0=33), 1, "replica0")]
    for kw, code, word in cases:
        rc, msg = xe(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        assert (rc, msg) == pc(**kw), kw                               # rrrmc_ctx_create_perc's checks, in its order, in its words
        assert "no HIP device" not in msg and "out of range (0.." not in msg
    for kw, code, word in cases[1:] + [(dict(sub=2), 1, "sub must be 0"), (dict(kind=10), 1, "slice_kind must be"), (dict(kind=12), 1, "slice_kind must be")]:
        rc, msg = af(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        assert "no HIP device" not in msg and "out of range (0.." not in msg
    # the ensembles and GraphQuant refuse kind 11 as they refuse 7 and 10, in the same words
    for name, types, args in (("rrrmc_ctx_create_re", [I64, I64, I32, I64, I32, U32], lambda k: (33, 3, k, 4, 0, 0)),
                              ("rrrmc_ctx_create_le", [I64, I64, I32, I64, I32, U32], lambda k: (33, 3, k, 4, 0, 0)),
                              ("rrrmc_ctx_create_tle", [I64, I64, I32, I64, I32, U32], lambda k: (33, 3, k, 4, 0, 0)),
                              ("rrrmc_ctx_create_quant_pattern", [I32, I64, I64, I64, I64, I32, U32], lambda k: (k, 33, 0, 3, 4, 0, 0))):
        got = {k: _call(pkg, name, types, False, *args(k)) for k in (7, 10, 11)}
        assert got[11][0] == 1 and got[11][1] == got[10][1].replace("given: 10", "given: 11") == got[7][1].replace("given: 7", "given: 11"), (name, got)
    # the multi-device creator hands the same refusals on, for the three new selectors
    lib = pkg.lib()
    for model in (66, 100, 101):
        ctx = C.c_void_p()
        rc = lib.rrrmc_ctx_create_multi(C.byref(ctx), model, 20, 0, 0, 4, np.zeros(1, np.int32), 1, 0)
        assert rc == 1 and b"N must be odd" in lib.rrrmc_last_error(None) and ctx.value is None
    assert lib.rrrmc_set_loss_table(None, np.zeros(4), 4) == 1 and lib.rrrmc_perc_step_energy(None, np.zeros(1, np.int64)) == 1


# ---- header, _lib.py and Julia ------------------------------------------------------------------------------------------------------------
def test_header_python_and_julia_agree_on_the_new_surface(pkg):
    sigs = header_signatures()
    want = {"rrrmc_ctx_create_perc_xentr": ("int32_t", ["rrrmc_ctx**", "int64_t", "int64_t", "int32_t", "uint32_t"]),
            "rrrmc_set_loss_table": ("int32_t", ["rrrmc_ctx*", "double*", "int64_t"]),
            "rrrmc_xentr_build": ("int32_t", ["rrrmc_ctx*", "int32_t*"]),
            "rrrmc_perc_step_energy": ("int32_t", ["rrrmc_ctx*", "int64_t*"])}
    for name, sig in want.items():
        assert sigs[name] == sig and name in pkg.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "rrrmc_hip.h"), encoding="utf-8").read()
    enum = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"RRRMC_(MODEL_\w*XENTR\w*|RE_SLICE_PERC_XENTR) = (\d+)", hdr))
    assert enum == {"MODEL_PERC_XENTR": 66, "MODEL_XENTR_AF": 100, "MODEL_XENTR_ASF": 101, "RE_SLICE_PERC_XENTR": 11}
    assert pkg.GraphPercXEntr.model_kind == 66
    bound = {c[0] for c in julia_ccalls(os.path.join(ROOT, "julia", "RRRMCHip.jl"))}
    assert set(want) <= bound
    jl = open(os.path.join(ROOT, "julia", "RRRMCHip.jl"), encoding="utf-8").read()
    assert re.search(r"const PERC_XENTR\s*=\s*66\b", jl) and re.search(r"const XENTR_AF, XENTR_ASF\s*=\s*100, 101\b", jl)
    assert "X.Hs" in jl                                                # the Julia binding passes the graph's own table


# ---- the Boltzmann law on 5 synapses ------------------------------------------------------------------------------------------------------
# N = 5, P = 3: 32 states.  β and the iteration count are shared with the GPU twin.  boltzmann_law.CASES has no perceptron row to take them
# from: β = 0.6 is the β of the repository's one Boltzmann test on GraphPercLinear (tests/test_gpu_perc.py), and 500 iterations are 100
# sweeps of the 5 synapses — at β = 0.6 every move of this instance is accepted with probability >= exp(-0.6 · 9) and most with far more,
# so the chain forgets its start within a few sweeps; the table's standardMC rows take 300 sweeps of 8 or 9 spins, which this twin's pure
# Python loop cannot afford.  BL_LAMBDA = 1.0 and the pattern seed give >= 5 distinct energies (asserted).  The CPU twin runs fewer chains
# and therefore tells a coarser error in β apart (CPU_POWER), as the twins of tests/test_add_fields_cpu.py and boltzmann_law.CASES (cpu_R,
# cpu_power) do; with these every pooled tail (β and CPU_POWER β) expects at least 5 chains.
BL_N, BL_P, BL_LAMBDA, BL_PATTERN_SEED = 5, 3, 1.0, 2
BL_BETA, BL_ITERS = 0.6, 500
BL_SEEDS = {"std-thread": 171, "std-wave": 172, "rrr-asf": 173}
BL_CPU_R, BL_CPU_POWER = 1024, 1.5


def bl_graph(pkg):
    return pkg.GraphPercXEntr(BL_N, BL_P, BL_LAMBDA, seed=BL_PATTERN_SEED)


def bl_fields():
    """the fields of the GraphAddSubFields twin (they shape the proposals only)"""
    return np.array([0.5, -1.0, 0.0, 1.0, -0.5])


def energy_from_definition(xi, lam, sg):
    """Σ_a log(1 + exp(−2λ σ·ξ_a / √N)) for every state in `sg` ([S, N] of ±1), from the docstring of PercXEntr.jl:74-84 — no table"""
    xi = 2 * np.asarray(xi, np.int64) - 1
    N = xi.shape[1]
    return np.log1p(np.exp(-2.0 * lam * (sg @ xi.T) / np.sqrt(N))).sum(axis=1)


def bl_energies(X):
    E = energy_from_definition(X.patterns(), X.lam, 2 * BL.enumerate_states(X.N) - 1)
    assert len(BL.energy_levels(E)[0]) >= 5
    return E


@pytest.mark.parametrize("which", ["std-thread", "rrr-asf"])
def test_the_restatement_follows_the_boltzmann_law(pkg, oracle, which):
    import add_fields_reference as AF
    X = bl_graph(pkg)
    xi, E = X.patterns(), bl_energies(X)
    seed = BL_SEEDS[which]
    case = BL._case("%s-GraphPercXEntr-5-3-restatement" % which, None, "rrr" if which == "rrr-asf" else "std", BL_BETA, BL_ITERS, seed, R=BL_CPU_R)
    chunks = np.zeros((BL_CPU_R, 1), np.uint64)
    for r in range(BL_CPU_R):
        s = ((int(oracle.init_config(seed, r, BL_N)[0]) >> np.arange(BL_N)) & 1).astype(np.int64)
        if which == "rrr-asf":
            run = AF.AfRun(AF.AddFields(bl_fields(), XR.PercXEntrRef(xi, BL_LAMBDA), True), s, BL_BETA, seed, oracle, replica=r)
            run.run(BL_ITERS, BL_ITERS)
            Etr = run.E
        else:
            _, Etr, _ = XR.standard_mc(XR.PercXEntrRef(xi, BL_LAMBDA), s, BL_BETA, BL_ITERS, BL_ITERS, seed, oracle, replica=r)
        chunks[r, 0] = sum(int(b) << j for j, b in enumerate(s))
        idx = BL.state_index_of_chunks(chunks[r:r + 1], BL_N)
        assert abs(Etr - E[idx[0]]) <= 1e-12 * max(1.0, abs(E[idx[0]]))
    v = BL.judge(case, E, BL.state_index_of_chunks(chunks, BL_N), None, power=BL_CPU_POWER)
    print("chi2 %s: law %.1f (limit %.1f, %d dof), at %.1f beta %.1f (limit %.1f)" % (case.id, v.law.chi2, v.law.limit, v.law.dof, BL_CPU_POWER, v.power.chi2, v.power.limit))
    BL.assert_verdict(v)
