"""GPU parity for the Topological Local Entropy ensemble (src/graphs/TLE.jl): rrrMC(X::DoubleGraph) and standardMC through the HIP kernels
equal the plain-Python restatement (tests/tle_reference.py) bit for bit — energies, final configuration, accepted / staged counts, the
DeltaECache's classes and set sizes, tracked and fresh energy(X, C), TLEenergies, cenergy and distances — over neighbourhoods wider than a
wavefront, more classes than a wavefront, degenerate tables, SAT slices, both builds, resumed and two-device runs; and the kernels' bounds
are enforced."""
import ctypes as C
import os

import numpy as np
import pytest

import le_reference as LE
import sat_reference as SR
import tle_reference as TLE

pytestmark = pytest.mark.gpu


def _graph(pkg, oracle, kind, Nk, M, gamma, lam, beta_g, seed, sat=None):
    """(the device graph, a factory of fresh reference graphs)"""
    if kind == "empty":
        X, J = pkg.Graph0TLE(Nk, M, gamma, lam, beta_g), None
    elif kind == "sk":
        X = pkg.GraphSKTLE(Nk, M, gamma, lam, beta_g, seed=seed)
        assert (X.J == oracle.gen_sk_binary(Nk, seed)).all()
        J = X.J
    elif kind == "skn":
        J = oracle.gen_sk_gauss(Nk, seed)
        X = pkg.GraphTopologicalLocalEntropy(Nk, M, gamma, lam, beta_g, pkg.GraphSKNormal.from_J(J))
    else:
        J = None
        X = pkg.GraphSATTLE(pkg.GraphSAT.from_clauses(*sat), M, gamma, lam, beta_g)
    return X, lambda: TLE.TopologicalLocalEntropy(Nk, M, gamma, lam, beta_g, kind, J, sat)


def _check_observables(eng, R, ref, configs):
    Es, Ec, D = eng.le_energies(), eng.cenergy(), eng.distances()
    X = ref()
    for r, s in configs:
        assert np.asarray(Es if R == 1 else Es[r]).tolist() == TLE.tle_energies(X, s)
        assert float(Ec if R == 1 else Ec[r]) == TLE.cenergy(X, s)
        assert np.asarray(D if R == 1 else D[r]).tolist() == TLE.distances(X.Nk, X.M, s)


def _check_rrr(pkg, oracle, kind, Nk, M, gamma, lam, beta_g, beta, R, iters, step, thr, check_reps=None, calls=1, sat=None, resume=False, devices=None,
               debug=False):
    seed = 7120041 + 31 * Nk + M
    X, ref = _graph(pkg, oracle, kind, Nk, M, gamma, lam, beta_g, seed, sat)
    N = Nk * (M + 1)
    with pkg.Engine(X, R, devices=devices) as eng:
        if debug:
            eng.set_debug_checks(True)
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        E0 = eng.energy()
        if resume:
            eng.set_resume(True)
        outs = []
        for c in range(calls):
            Es, acc, staged = eng.rrr_mc(beta, iters, step, staged_thr=thr)
            outs.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config(), eng.tle_cache(), eng.run_energy()))
        reps = list(check_reps if check_reps is not None else range(R))
        finals = {}
        if resume:
            eng.set_resume(False)
        Ef = eng.energy()
        for r in reps:
            s = TLE.config_from_chunks(C0.s[r], N)
            assert (C0.s[r] == oracle.init_config(seed, r, N)).all()
            assert E0[r] == TLE.energy_fresh(ref(), s)
            run = None
            for c in range(calls):
                if run is None or not resume:          # a resumed call continues the run; otherwise a call starts like a reference call
                    run = TLE.RrrRun(ref(), s, beta, seed, oracle, replica=r, it0=c * iters, staged_thr=thr)
                    acc0 = st0 = 0
                else:
                    acc0, st0 = run.accepted, run.staged_its
                es = run.run(iters, step)
                Es, acc, staged, C1, (pos, sizes), Etr = outs[c]
                assert np.asarray(Es[r]).tolist() == es, (r, c)
                assert acc[r] == run.accepted - acc0 and staged[r] == run.staged_its - st0, (r, c)
                assert (C1.s[r] == TLE.chunks_from_config(s)).all(), (r, c)
                p_ref, sz_ref = run.cache_view()
                assert (pos[r] == p_ref).all() and (sizes[r] == sz_ref).all(), (r, c)
                assert Etr[r] == run.E
            assert Ef[r] == TLE.energy_fresh(ref(), s)
            finals[r] = s
        _check_observables(eng, R, ref, finals.items())
        return outs


@pytest.mark.parametrize("kind", ["sk", "skn"])
@pytest.mark.parametrize("thr", [0.5, 0.0, 1.0])
def test_rrr_tle_neighbour_phase_wider_than_a_wavefront(pkg, oracle, kind, thr):
    # Nk = 10, M = 8 over all-to-all slices: a centre move has 8 + 9 * 9 = 89 neighbours
    _check_rrr(pkg, oracle, kind, 10, 8, 1.5, 0.5, 2.0, 2.0, 2, 2500, 100, thr)


def test_rrr_tle_more_classes_than_a_wavefront(pkg, oracle):
    X = pkg.GraphSKTLE(10, 3, 0.9, 0.37, 1.0, seed=1)
    assert 2 * len(X.tables()) > 64
    _check_rrr(pkg, oracle, "sk", 10, 3, 0.9, 0.37, 1.0, 1.3, 3, 4000, 100, 0.5)


@pytest.mark.parametrize("kind,Nk,M,R", [("sk", 13, 5, 1), ("skn", 9, 4, 3), ("empty", 37, 3, 70), ("sk", 11, 6, 70)])
def test_rrr_tle_odd_even_M_unaligned_many_replicas(pkg, oracle, kind, Nk, M, R):
    _check_rrr(pkg, oracle, kind, Nk, M, 1.0, 0.5, 1.0, 1.5, R, 2500, 250, 0.5, check_reps=[0, 1, R - 1] if R > 3 else None, calls=2)


@pytest.mark.parametrize("gamma,lam", [(1.1, 0.0), (0.0, 0.8), (0.7, 0.7), (0.6, -0.4)])
def test_rrr_tle_degenerate_tables(pkg, oracle, gamma, lam):
    _check_rrr(pkg, oracle, "sk", 7, 4, gamma, lam, 1.2, 0.9, 2, 3000, 100, 0.5)


def test_rrr_tle_sat_ragged_clauses_and_isolated_variable(pkg, oracle):
    # variable 0 shares clauses with 18 others (a centre move: 3 + 4 * 18 = 75 neighbours), variable 19 is in no clause (∂i empty)
    sat = SR.ragged_instance()
    nb = SR.ClauseCache(*sat).neighb
    assert nb[19] == [] and len(nb[0]) == 18
    _check_rrr(pkg, oracle, "sat", 20, 3, 0.6, 0.4, 1.2, 0.8, 2, 3000, 100, 0.5, sat=sat)


def test_rrr_tle_random_3sat(pkg, oracle):
    S = pkg.GraphSAT(20, 3, 4.2, seed=11)
    _check_rrr(pkg, oracle, "sat", 20, 3, 0.6, 0.4, 1.2, 0.8, 2, 3000, 100, 0.5, sat=(20, S.A, S.J))


def test_graph0tle_equals_graph0le(pkg):
    # no neighbours: lfields2 = 0 and the two models coincide, level for level
    res = []
    for X in (pkg.Graph0TLE(21, 6, 1.2, 0.45, 1.0), pkg.Graph0LE(21, 6, 1.2, 1.0)):
        with pkg.Engine(X, 3) as eng:
            eng.seed(99)
            eng.init_spins_random()
            E0 = eng.energy()
            out = eng.rrr_mc(1.7, 5000, 50)
            pos, sizes = eng.tle_cache() if X.model_kind == 44 else eng.rrr_cache()
            std = eng.standard_mc(1.7, 3000, 50)
            res.append((E0, out, eng.get_config().s.copy(), pos.astype(np.int64), sizes, std))
    (Ea, a, ca, pa, sa, ta), (Eb, b, cb, pb, sb, tb) = res
    assert (Ea == Eb).all() and (ca == cb).all() and (pa == pb).all() and (sa == sb).all()
    for x, y in zip(a + ta, b + tb):
        assert (np.asarray(x) == np.asarray(y)).all()


@pytest.mark.parametrize("kind", ["sk", "skn", "sat"])
def test_rrr_tle_lds_and_global_builds_agree(pkg, kind):
    S = pkg.GraphSAT(21, 3, 4.2, seed=3)
    X = pkg.GraphSKTLE(21, 6, 1.2, 0.3, 1.0, seed=3) if kind == "sk" else pkg.GraphSATTLE(S, 4, 1.2, 0.3, 1.0) if kind == "sat" else \
        pkg.GraphTopologicalLocalEntropy(21, 7, 1.2, 0.3, 1.0, pkg.GraphSKNormal(21, seed=3))
    res = []
    for no_lds, build in (("1", 2), ("0", 1)):
        old = os.environ.get("RRRMC_TLE_NO_LDS")
        os.environ["RRRMC_TLE_NO_LDS"] = no_lds
        try:
            with pkg.Engine(X, 5) as eng:
                eng.seed(99)
                eng.init_spins_random()
                assert eng.tle_build() == 0
                out = eng.rrr_mc(1.7, 5000, 50)
                assert eng.tle_build() == build
                res.append((out, eng.get_config().s.copy(), eng.tle_cache(), eng.run_energy()))
        finally:
            if old is None:
                os.environ.pop("RRRMC_TLE_NO_LDS", None)
            else:
                os.environ["RRRMC_TLE_NO_LDS"] = old
    (a, ca, pa, ea), (b, cb, pb, eb) = res
    for x, y in zip(a, b):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert (ca == cb).all() and (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all() and (ea == eb).all()


def test_rrr_tle_two_resumed_calls_equal_one_call(pkg, oracle):
    two = _check_rrr(pkg, oracle, "sk", 9, 4, 1.0, 0.5, 1.0, 1.4, 2, 1500, 100, 0.5, calls=2, resume=True)
    one = _check_rrr(pkg, oracle, "sk", 9, 4, 1.0, 0.5, 1.0, 1.4, 2, 3000, 100, 0.5, check_reps=[])
    assert np.concatenate([two[0][0], two[1][0]], axis=1).tolist() == one[0][0].tolist()
    assert (two[1][3].s == one[0][3].s).all() and (two[0][1] + two[1][1] == one[0][1]).all()
    assert (two[1][4][0] == one[0][4][0]).all() and (two[1][5] == one[0][5]).all()


def test_rrr_tle_two_device_context_equals_one_device(pkg, oracle):
    a = _check_rrr(pkg, oracle, "sk", 9, 4, 1.0, 0.5, 1.0, 1.4, 70, 1500, 100, 0.5, check_reps=[0, 69], devices=[0, 0])
    b = _check_rrr(pkg, oracle, "sk", 9, 4, 1.0, 0.5, 1.0, 1.4, 70, 1500, 100, 0.5, check_reps=[])
    assert a[0][0].tolist() == b[0][0].tolist() and (a[0][3].s == b[0][3].s).all()
    assert (a[0][4][0] == b[0][4][0]).all() and (a[0][4][1] == b[0][4][1]).all()


@pytest.mark.parametrize("kind", ["sk", "skn", "sat", "empty"])
def test_tle_debug_switch_passes(pkg, oracle, kind):
    sat = SR.ragged_instance() if kind == "sat" else None
    Nk = 20 if kind == "sat" else 12
    X, _ = _graph(pkg, oracle, kind, Nk, 5, 0.8, 0.3, 1.0, 77, sat)
    with pkg.Engine(X, 3) as eng:
        eng.set_debug_checks(True)
        eng.seed(5)
        eng.init_spins_random()
        eng.rrr_mc(1.1, 3000, 100)
        eng.rrr_mc(1.1, 3000, 100, staged_thr=1.0)
        eng.standard_mc(1.1, 3000, 100)
        eng.sync()
        Etr, E = eng.run_energy(), eng.energy()
        assert (np.abs(Etr - E) <= 1e-10 * np.maximum(1.0, np.abs(E))).all()


@pytest.mark.parametrize("kind,M", [("empty", 5), ("sk", 4), ("skn", 5), ("sk", 8), ("sat", 3)])
def test_standard_tle_bit_exact(pkg, oracle, kind, M):
    sat = SR.ragged_instance() if kind == "sat" else None
    Nk, gamma, lam, beta_g, beta, R = (20 if kind == "sat" else 11), 1.5, 0.5, 2.0, 1.2, 3
    seed = 5511 + M
    X, ref = _graph(pkg, oracle, kind, Nk, M, gamma, lam, beta_g, seed, sat)
    N = Nk * (M + 1)
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        Es, acc = eng.standard_mc(beta, 4000, 100)
        C1 = eng.get_config()
        Etr = eng.run_energy()
        finals = []
        for r in range(R):
            s = TLE.config_from_chunks(C0.s[r], N)
            es, E, a = TLE.standard_mc(ref(), s, beta, 4000, 100, seed, oracle, replica=r)
            assert Es[r].tolist() == [float(e) for e in es] and acc[r] == a
            assert (C1.s[r] == TLE.chunks_from_config(s)).all()
            assert Etr[r] == E
            finals.append((r, s))
        _check_observables(eng, R, ref, finals)


def test_tle_bounds_and_refusals(pkg):
    L = pkg.lib()
    ctx = C.c_void_p()
    assert L.rrrmc_ctx_create_tle(C.byref(ctx), 10, 2, 0, 4, 0, 0) == 1                  # M > 2 (TLE.jl:29)
    assert L.rrrmc_ctx_create_tle(C.byref(ctx), 10, 32, 0, 4, 0, 0) == 3                 # M <= 31
    assert b"M <= 31" in L.rrrmc_last_error(None)
    assert L.rrrmc_ctx_create_tle(C.byref(ctx), 8192, 7, 0, 4, 0, 0) == 3                # N = 65 536 > 65 535
    assert b"65535" in L.rrrmc_last_error(None)
    assert L.rrrmc_ctx_create_tle(C.byref(ctx), 10, 5, 7, 4, 0, 0) == 1                  # slice kind 7 is unassigned
    for kind in (3, 4, 5, 6, 9):
        assert L.rrrmc_ctx_create_tle(C.byref(ctx), 15, 5, kind, 4, 0, 0) == 3           # perceptron and committee slices: not covered
    assert L.rrrmc_ctx_create(C.byref(ctx), 44, 60, 0, 4, 0, 0) != 0                     # the TLE selectors are rrrmc_ctx_create_multi's
    X = pkg.GraphSKTLE(10, 5, 1.0, 0.5, 1.0, seed=1)
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call in (lambda: eng.bkl_mc(1.0, 100, 10), lambda: eng.wtm_mc(1.0, 10, 1.0), lambda: eng.extremal_opt(1.4, 100, 10)):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3
        eng.rrr_mc(1.0, 100, 10)
        with pytest.raises(pkg.RRRMCError):
            eng.rrr_cache()                                                              # int8 class ids: not served
        assert L.rrrmc_le_set_params(eng._ctx, 1.0, 1.0) == 2                            # not a Local Entropy context
        assert L.rrrmc_tle_set_params(eng._ctx, 1.0, 1.0, 0.0) == 1                      # γ / β not finite
        bad = np.array([0, 1] + [1] * 9, np.int32), np.array([3], np.int32)              # ∂0 = {3}, ∂3 = {}: not symmetrical
        assert L.rrrmc_tle_set_topology(eng._ctx, *bad) == 1
        assert b"not symmetrical" in L.rrrmc_last_error(eng._ctx)
    with pkg.Engine(pkg.Graph0LE(10, 5, 1.0, 1.0), 2) as eng:
        assert L.rrrmc_tle_set_params(eng._ctx, 1.0, 1.0, 1.0) == 2                      # not a TLE context
