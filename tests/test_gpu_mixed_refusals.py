"""What a GraphMixed context refuses on the device, by name: a second component of a storage group, unequal N, K = 9, a parity that one
component's rule forbids, rrrMC on the stand-alone mix, bklMC / wtmMC / extremal_opt, a sampling or energy call before every upload is
there, the field calls on the stand-alone mix, and rrrmc_ctx_create_af with RRRMC_RE_SLICE_MIXED."""
import ctypes as C

import numpy as np
import pytest

import mixed_instances as MI

pytestmark = pytest.mark.gpu

SK, SKN, PL, CR, SAT, PX, SPF, MIXED = 1, 2, 4, 6, 8, 11, 12, 13


def _create(pkg, kinds, wrap=0, N=15, K=0, K2=0, R=4):
    lib = pkg.lib()
    ctx = C.c_void_p()
    k = np.asarray(kinds, np.int32)
    rc = lib.rrrmc_ctx_create_mixed(C.byref(ctx), k, len(k), wrap, N, K, K2, R, 0, 0)
    msg = lib.rrrmc_last_error(None)
    return int(rc), (msg.decode() if msg else ""), ctx


def test_create_time_refusals(pkg):
    for kw, code, word in [
        (dict(kinds=[SK, SAT, SK]), 3, "storage group {SK}"),
        (dict(kinds=[SPF, SK], K=9), 3, "cover K <= 8"),
        (dict(kinds=[PL, CR], N=8, K2=2), 1, "component 0 (a perceptron): N must be odd"),
        (dict(kinds=[PL, CR], N=15, K2=3), 1, "component 1 (a committee machine): K1 must be even"),
    ]:
        rc, msg, ctx = _create(pkg, **kw)
        assert rc == code and word in msg and ctx.value is None, (kw, rc, msg)
    ctx = C.c_void_p()
    assert pkg.lib().rrrmc_ctx_create_af(C.byref(ctx), MIXED, 0, 15, 0, 4, 0, 0) == 1 and ctx.value is None
    assert b"slice_kind must be" in pkg.lib().rrrmc_last_error(None)
    with pytest.raises(ValueError, match="same N for all graphs required"):
        pkg.GraphMixed(pkg.GraphSK(15), pkg.GraphSAT(16, 3, 4.2))
    with pytest.raises(NotImplementedError, match="storage group"):
        pkg.GraphMixed(pkg.GraphSK(15), pkg.GraphSAT(15, 3, 4.2), pkg.GraphSK(15, seed=2))


def test_sampling_before_every_upload_names_the_missing_call(pkg):
    lib = pkg.lib()
    rc, msg, ctx = _create(pkg, [PX, SK, SAT], N=33)
    assert rc == 0 and ctx.value
    try:
        lib.rrrmc_seed(ctx, 1)
        assert lib.rrrmc_init_spins_random(ctx) == 0
        g = pkg.GraphPercXEntr(33, 5, 0.8)
        sk, sat = pkg.GraphSK(33), pkg.GraphSAT(33, 3, 4.2)
        E = np.zeros(4)
        for upload, missing in ((None, "rrrmc_set_couplings_bits"), (lambda: sk._upload_couplings(ctx), "rrrmc_set_patterns"),
                                (lambda: pkg.lib().rrrmc_set_patterns(ctx, g.xi.reshape(-1), g.P), "rrrmc_set_clauses"),
                                (lambda: sat._upload_couplings(ctx), "rrrmc_set_loss_table")):
            if upload is not None:
                assert upload() in (None, 0)
            assert lib.rrrmc_standard_mc_async(ctx, 1.0, 10, 1) == 2 and missing in lib.rrrmc_last_error(ctx).decode()
            assert lib.rrrmc_energy_f64(ctx, E) == 2 and missing in lib.rrrmc_last_error(ctx).decode()
            assert lib.rrrmc_mixed_energies(ctx, np.zeros(12)) == 2
        assert lib.rrrmc_set_loss_table(ctx, g.Hs, len(g.Hs)) == 0
        assert lib.rrrmc_energy_f64(ctx, E) == 0 and lib.rrrmc_standard_mc_async(ctx, 1.0, 10, 1) == 0 and lib.rrrmc_sync(ctx) == 0
        # an upload that does not belong to the list is refused
        assert lib.rrrmc_set_couplings_dense(ctx, np.zeros(33 * 33)) == 2
        # the stand-alone mix has no fields
        assert lib.rrrmc_af_set_fields(ctx, np.zeros(33)) == 2 and b"wrap 1 or 2" in lib.rrrmc_last_error(ctx)
        b = C.c_int32(0)
        assert lib.rrrmc_af_build(ctx, C.byref(b)) == 2
    finally:
        lib.rrrmc_ctx_destroy(ctx)


def test_a_wrapper_needs_its_fields(pkg):
    lib = pkg.lib()
    rc, msg, ctx = _create(pkg, [SK, SAT], wrap=2)
    assert rc == 0
    try:
        lib.rrrmc_seed(ctx, 1)
        lib.rrrmc_init_spins_random(ctx)
        pkg.GraphSK(15)._upload_couplings(ctx)
        pkg.GraphSAT(15, 3, 4.2)._upload_couplings(ctx)
        assert lib.rrrmc_standard_mc_async(ctx, 1.0, 10, 1) == 2 and b"rrrmc_af_set_fields" in lib.rrrmc_last_error(ctx)
        assert b"GraphMixed" in lib.rrrmc_last_error(ctx)
    finally:
        lib.rrrmc_ctx_destroy(ctx)


def test_what_is_not_wired_is_refused(pkg):
    X = MI.mix(pkg, "int21")
    with pkg.Engine(X, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        with pytest.raises(pkg.RRRMCError) as e:
            eng.rrr_mc(1.0, 10)
        assert e.value.code == 3 and "GraphMixed" in str(e.value) and "GraphAddFields / GraphAddSubFields" in str(e.value)
        for call, word in ((lambda: eng.bkl_mc(1.0, 10), "bklMC"), (lambda: eng.wtm_mc(1.0, 2), "wtmMC"), (lambda: eng.extremal_opt(1.2, 10), "extremal_opt")):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3 and word in str(e.value) and "GraphMixed" in str(e.value)
        Es, acc = eng.standard_mc(1.0, 10, 1)          # the context is still usable
        assert np.atleast_2d(Es).shape == (2, 10)
    Xw = pkg.GraphAddFields(MI.fields(21), X)
    with pkg.Engine(Xw, 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        for call, word in ((lambda: eng.bkl_mc(1.0, 10), "bklMC"), (lambda: eng.wtm_mc(1.0, 2), "wtmMC"), (lambda: eng.extremal_opt(1.2, 10), "extremal_opt")):
            with pytest.raises(pkg.RRRMCError) as e:
                call()
            assert e.value.code == 3 and word in str(e.value) and "GraphAddFields over a GraphMixed" in str(e.value)
        eng.rrr_mc(1.0, 10)
