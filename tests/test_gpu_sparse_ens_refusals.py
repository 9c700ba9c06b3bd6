"""What the ensembles over sparse Float64 slices refuse, with which code and in which words: slice kind 12 through the creators that carry no
K, K out of range, M <= 2 and M beyond the kernels, N > 65 535, non-finite couplings, unsorted or asymmetric (A, J), samplers before the graph
or the parameters, and the samplers that are not wired.  Every refusal is made on the host: nothing here launches a kernel on bad input."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID_ARG, STATE, UNSUPPORTED = 1, 2, 3
FAMS = ("re", "le", "tle")


def _err(L, ctx=None):
    m = L.rrrmc_last_error(ctx)
    return m.decode() if m else ""


def _f64(L, fam):
    return getattr(L, "rrrmc_ctx_create_%s_f64" % fam)


@pytest.mark.parametrize("fam", FAMS)
def test_creators(pkg, fam):
    L = pkg.lib()
    ctx = C.c_void_p()
    old = getattr(L, "rrrmc_ctx_create_" + fam)
    # kind 12 through the creator without a K: a message of its own that names the _f64 creator
    assert old(C.byref(ctx), 9, 3, 12, 2, 0, 0) == INVALID_ARG and ctx.value is None
    assert _err(L) == "slice_kind RRRMC_RE_SLICE_SPARSE_F64 needs the K of the slice graph: use rrrmc_ctx_create_%s_f64" % fam
    # ... and the pinned wording for every other bad kind stays
    assert old(C.byref(ctx), 9, 3, 13, 2, 0, 0) == INVALID_ARG
    assert _err(L).startswith("slice_kind must be ") and _err(L).endswith("given: 13")
    new = _f64(L, fam)
    for K, code, text in ((0, INVALID_ARG, "Nk, K, R must be >= 1"), (-1, INVALID_ARG, "Nk, K, R must be >= 1"),
                          (9, UNSUPPORTED, "K=9: the Float64 sparse slice kernels cover K <= 8")):
        assert new(C.byref(ctx), 9, K, 3, 2, 0, 0) == code and ctx.value is None, K
        assert _err(L) == text
    assert new(C.byref(ctx), 0, 4, 3, 2, 0, 0) == INVALID_ARG and _err(L) == "Nk and R must be >= 1"
    for M in (2, 0):
        assert new(C.byref(ctx), 9, 4, M, 2, 0, 0) == INVALID_ARG and _err(L) == "M must be greater than 2, given: %d" % M
    Mmax = 32 if fam == "re" else 31
    assert new(C.byref(ctx), 9, 4, Mmax + 1, 2, 0, 0) == UNSUPPORTED and ("M = %d: " % (Mmax + 1)) in _err(L) and ("M <= %d" % Mmax) in _err(L)
    rows = 4 if fam == "re" else 3                   # Nk M (RE) or Nk (M + 1) (LE, TLE) = 65 536
    assert new(C.byref(ctx), 16384, 4, rows, 2, 0, 0) == UNSUPPORTED and "N <= 65535" in _err(L) and "65536" in _err(L)
    assert new(C.byref(ctx), 9, 4, 3, 2, 0, 16) == INVALID_ARG and "replica0 must be a multiple of 32" in _err(L)
    assert ctx.value is None
    # the largest K is taken
    assert new(C.byref(ctx), 9, 8, 3, 2, 0, 0) == 0 and ctx.value
    L.rrrmc_ctx_destroy(ctx)


@pytest.mark.parametrize("fam", FAMS)
def test_graph_checks_and_call_order(pkg, fam):
    L = pkg.lib()
    X = pkg.GraphEARE(3, 2, 3, 1.0, 1.0, seed=2).X1
    A, J = X.A, X.J
    ctx = C.c_void_p()
    assert _f64(L, fam)(C.byref(ctx), 9, 4, 3, 2, 0, 0) == 0
    try:
        assert L.rrrmc_seed(ctx, 5) == 0 and L.rrrmc_init_spins_random(ctx) == 0
        # samplers before the graph
        assert L.rrrmc_rrr_mc_async(ctx, 1.0, 1.0, 100, 10, 0.5, 5.0) == STATE and _err(L, ctx) == "rrrmc_set_graph has not been called"
        assert L.rrrmc_standard_mc_async(ctx, 1.0, 100, 10) == STATE and _err(L, ctx) == "rrrmc_set_graph has not been called"

        def refused(A_, J_, text):
            assert L.rrrmc_set_graph_f64(ctx, np.ascontiguousarray(A_, np.int32), np.ascontiguousarray(J_, np.float64).reshape(-1)) == INVALID_ARG
            assert text in _err(L, ctx), _err(L, ctx)
        for bad in (np.inf, -np.inf, np.nan):
            Jb = J.copy()
            Jb[3, 1] = bad
            refused(A, Jb, "J[13] is not finite")
        Ab = A.copy()
        Ab[4] = Ab[4][::-1]
        refused(Ab, J, "row 4 of A is not sorted")
        Ab = A.copy()
        Ab[0, 0] = 9
        refused(Ab, J, "out of range 0..8")
        Jb = J.copy()
        Jb[0, 0] += 0.5
        refused(A, Jb, "is not symmetric in (A, J)")
        Ab = A.copy()
        Ab[0] = np.sort(np.r_[Ab[0][:3], 0])
        refused(Ab, J, "self loop at site 0")
        # the graph given, the parameters not: the samplers still refuse
        assert L.rrrmc_set_graph_f64(ctx, A, J.reshape(-1)) == 0
        assert L.rrrmc_rrr_mc_async(ctx, 1.0, 1.0, 100, 10, 0.5, 5.0) == STATE
        want = ("rrrmc_tle_set_topology and rrrmc_tle_set_params first" if fam == "tle" else "call rrrmc_%s_set_params first" % fam)
        assert want in _err(L, ctx)
        assert L.rrrmc_standard_mc_async(ctx, 1.0, 100, 10) == STATE and want in _err(L, ctx)
        if fam == "tle":
            assert L.rrrmc_tle_set_params(ctx, 1.0, 0.5, 1.0) == STATE and "comes after rrrmc_tle_set_topology" in _err(L, ctx)
            # row A[i] with its duplicates is no topology: the lists are uA
            A2 = pkg.GraphEARE(2, 2, 3, 1.0, 1.0, seed=2).X1.A
            ctx2 = C.c_void_p()
            assert _f64(L, fam)(C.byref(ctx2), 4, 4, 3, 2, 0, 0) == 0
            rowptr = np.arange(0, 17, 4, dtype=np.int32)
            assert L.rrrmc_tle_set_topology(ctx2, rowptr, np.ascontiguousarray(A2.reshape(-1))) == INVALID_ARG
            assert "duplicated element 1 in neighb[1]" in _err(L, ctx2)
            L.rrrmc_ctx_destroy(ctx2)
        # a context of another family does not take the call
        other = C.c_void_p()
        assert L.rrrmc_ctx_create_re(C.byref(other), 9, 3, 0, 2, 0, 0) == 0
        assert L.rrrmc_set_graph_f64(other, A, J.reshape(-1)) == STATE and "rrrmc_set_graph_f64 is for" in _err(L, other)
        L.rrrmc_ctx_destroy(other)
    finally:
        L.rrrmc_ctx_destroy(ctx)


@pytest.mark.parametrize("fam", FAMS)
def test_samplers_that_are_not_wired(pkg, fam):
    X = (pkg.GraphEARE(3, 2, 3, 1.0, 1.0) if fam == "re" else pkg.GraphEALE(3, 2, 3, 1.0, 1.0) if fam == "le" else pkg.GraphEATLE(3, 2, 3, 1.0, 0.5, 1.0))
    name = {"re": "GraphRobustEnsemble", "le": "GraphLocalEntropy", "tle": "GraphTopologicalLocalEntropy"}[fam]
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for sampler, call in (("bklMC", lambda: eng.bkl_mc(1.0, 100, 10)), ("wtmMC", lambda: eng.wtm_mc(1.0, 10, 1.0)),
                              ("extremal_opt", lambda: eng.extremal_opt(1.4, 100, 10))):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == UNSUPPORTED
            assert "%s is not wired for the %s (rrrMC and standardMC are)" % (sampler, name) in str(e.value)


def test_front_end_refuses_an_l1_lattice_for_the_tle(pkg):
    # L = 1: every site is its own neighbour; GraphTLE's constructor refuses a list that contains itself (TLE.jl:36)
    with pytest.raises((ValueError, pkg.RRRMCError)):
        pkg.GraphEATLE(1, 2, 3, 1.0, 0.5, 1.0)
