"""GPU checks of the cross-replica overlaps (rrrmc_cross_overlaps, rrrmc_overlap_hist, parsexovs): every spin layout against the numpy
reference of tests/xov_reference.py, at the smallest shapes where each piece can go wrong — tail bits beyond N, a partial 32-replica
group, a partial 64 x 64 tile, more words than one LDS slab and no multiple of it.  Every comparison is exact."""
import math
import os

import numpy as np
import pytest

import xov_reference as XR

pytestmark = pytest.mark.gpu

ENVS = ("RRRMC_XOV_NO_LDS_HIST", "RRRMC_XOV_PACK_BYTES")


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in ENVS}
    for k in ENVS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in ENVS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _graph(pkg, case, seed):
    if case == "rrg130":
        return pkg.GraphRRG(130, 3, seed=seed), 70              # bit-sliced: nch = 3, 2 tail bits, a partial 32-group and a partial tile
    if case == "sk65":
        return pkg.GraphSK(65, seed=seed), 9                    # 8 replicas per byte, a partial group
    if case == "rrgnormal130":
        return pkg.GraphRRGNormal(130, 3, seed=seed), 70        # 64-bit lanes
    if case == "sat100":
        return pkg.GraphSAT(100, 3, 4.2, seed=seed), 5          # chunk layout
    if case == "quant10x8":
        return pkg.GraphQuant(pkg.GraphRRG(10, 3, seed=seed), 8, 0.5, 2.0), 5      # N = Nk * M
    if case == "rrg2100":
        return pkg.GraphRRG(2100, 3, seed=seed), 33             # 33 words: two slabs and one word
    raise ValueError(case)


def _three_slots(eng, case, iters=400):
    """three snapshots with a short run at β = 1 between them, and one more run: the live configuration differs from all"""
    eng.snapshot_reserve(4)                                      # slot 3 stays empty
    for k in range(4):
        if case == "quant10x8":
            eng.rrr_mc(1.0, iters, iters)
        else:
            eng.standard_mc(1.0, iters, iters)
        if k < 3:
            eng.snapshot_store(k)
    return [eng.snapshot_get(k).bits() for k in range(3)] + [eng.get_config().bits()]      # index 3 = -1 = live


CASES = ["rrg130", "sk65", "rrgnormal130", "sat100", "quant10x8", "rrg2100"]


@pytest.mark.parametrize("case", CASES)
def test_matrix_and_histogram_match_the_reference(pkg, case):
    seed = 424200 + CASES.index(case)
    X, R = _graph(pkg, case, seed)
    N = X.N
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        bits = _three_slots(eng, case)
        q = eng.cross_overlaps([0, 2, -1], [1, 2, 0])
        a0, nA, b0, nB = (1, R - 2, 2, R - 3) if R > 8 else (1, 3, 2, 2)
        sub = eng.cross_overlaps([0, 2, -1], [1, 2, 0], rowsA=(a0, nA), rowsB=(b0, nB))
        one = eng.cross_overlaps(0, 1)                           # scalars: one pair
        own = eng.overlaps([0, 2, -1], [1, 2, 0])
        pairs = [([2], [2]), ([0], [1]), ([2, 0, -1, 1], [2, 1, 0, 1])]
        hists = [eng.overlap_hist(a, b) for a, b in pairs]
        hists_global = _with_env({"RRRMC_XOV_NO_LDS_HIST": "1"}, lambda: [eng.overlap_hist(a, b) for a, b in pairs])
        hists_batched = _with_env({"RRRMC_XOV_PACK_BYTES": "1"}, lambda: [eng.overlap_hist(a, b) for a, b in pairs])
        q_batched = _with_env({"RRRMC_XOV_PACK_BYTES": "1"}, lambda: eng.cross_overlaps([0, 2, -1], [1, 2, 0]))
        live_after = eng.get_config().bits()
    assert (live_after == bits[3]).all()                         # the calls leave the configuration alone
    assert q.shape == (3, R, R) and q.dtype == np.int32 and sub.shape == (3, nA, nB) and one.shape == (1, R, R)
    want = [XR.cross_matrix(bits[a], bits[b], N) for a, b in ((0, 1), (2, 2), (3, 0))]
    for p in range(3):
        assert (q[p] == want[p]).all(), (case, p)
        assert (sub[p] == want[p][a0:a0 + nA, b0:b0 + nB]).all(), (case, p)
        assert (np.diagonal(q[p]) == own[p]).all()              # r1 == r2 is rrrmc_overlaps' two-time self overlap
    assert (one[0] == want[0]).all() and (q_batched == q).all()
    assert (q[1] == q[1].T).all() and (np.diagonal(q[1]) == N).all()
    assert len({tuple(b.reshape(-1)) for b in bits}) == 4       # the slots differ, so the cases above are not one case
    refs = [XR.hist([(bits[2], bits[2], True)], N), XR.hist([(bits[0], bits[1], False)], N),
            XR.hist([(bits[2], bits[2], True), (bits[0], bits[1], False), (bits[3], bits[0], False), (bits[1], bits[1], True)], N)]
    sums = [R * (R - 1) // 2, R * (R - 1), 3 * R * (R - 1)]
    for k in range(3):
        assert hists[k].shape == (N + 1,) and hists[k].dtype == np.int64
        assert (hists[k] == refs[k]).all(), (case, k)
        assert (hists_global[k] == refs[k]).all() and (hists_batched[k] == refs[k]).all(), (case, k)
        assert int(hists[k].sum()) == sums[k]
    m = pkg.overlap_moments(hists[0], N)
    ref_m = XR.moments([want[1][i, j] for i in range(R) for j in range(i + 1, R)], N)
    assert m["pairs"] == ref_m["pairs"] and m["q2"] == ref_m["q2"] and m["q4"] == ref_m["q4"] and m["absq"] == ref_m["absq"] and m["binder"] == ref_m["binder"]


def test_one_replica(pkg):
    X = pkg.GraphRRG(130, 3, seed=5)
    with pkg.Engine(X, 1) as eng:
        eng.seed(5)
        eng.init_spins_random()
        eng.snapshot_reserve(1)
        eng.snapshot_store(0)
        eng.standard_mc(1.0, 300, 300)
        q = eng.cross_overlaps([0, -1], [0, 0])
        h = eng.overlap_hist([0, -1], [0, 0])
        b0, b1 = eng.snapshot_get(0).bits(), eng.get_config().bits()
    assert q.shape == (2, 1, 1) and q[0, 0, 0] == 130 and q[1, 0, 0] == XR.cross_matrix(b1, b0, 130)[0, 0] and q[1, 0, 0] < 130
    assert h.shape == (131,) and not h.any()


def test_two_shards_give_the_single_context_results(pkg):
    seed, R = 9191, 70
    X = pkg.GraphRRG(130, 3, seed=seed)
    out = []
    for devs in (None, [0, 0]):
        with pkg.Engine(X, R, devices=devs) as eng:
            eng.seed(seed)
            eng.init_spins_random()
            bits = _three_slots(eng, "rrg130")
            out.append((bits, eng.cross_overlaps([0, 2, -1], [1, 2, 0]), eng.cross_overlaps([0, -1], [1, 2], rowsA=(30, 37), rowsB=(5, 64)),
                        eng.overlap_hist([2, 0, -1], [2, 1, 0]), _with_env({"RRRMC_XOV_NO_LDS_HIST": "1"}, lambda: eng.overlap_hist([2, 0, -1], [2, 1, 0]))))
    single, multi = out
    for k in range(4):
        assert (single[0][k] == multi[0][k]).all()
    bits = multi[0]
    want = [XR.cross_matrix(bits[a], bits[b], 130) for a, b in ((0, 1), (2, 2), (3, 0))]
    for p in range(3):
        assert (multi[1][p] == want[p]).all()
    assert (multi[2][0] == want[0][30:67, 5:69]).all() and (multi[2][1] == XR.cross_matrix(bits[3], bits[2], 130)[30:67, 5:69]).all()
    ref_h = XR.hist([(bits[2], bits[2], True), (bits[0], bits[1], False), (bits[3], bits[0], False)], 130)
    assert (multi[3] == ref_h).all() and (multi[4] == ref_h).all()
    for k in range(1, 5):
        assert (single[k] == multi[k]).all()


def _same_floats(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (math.isnan(x) and math.isnan(y)) or (x == y and math.copysign(1.0, x) == math.copysign(1.0, y)), (a, b)


def test_parsexovs_equals_the_literal_transcription(pkg):
    seed, N, R, step, nsamp = 78, 130, 6, 300, 12
    X = pkg.GraphRRG(N, 3, seed=seed)
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        log = pkg.SnapshotLog(eng, nsamp)
        pkg.standardMC(X, 1.0, step * nsamp, step=step, seed=seed, hook=log, quiet=True, engine=eng)
        assert log.count == nsamp
        # synthetic clocks (the real ones are machine-dependent): the second has a gap, so that one window [t, 2t) holds no sample
        ts1 = [float(k + 1) for k in range(nsamp)]
        ts2 = [1.0, 2.0, 3.0] + [float(k + 7) for k in range(3, nsamp)]
        got = {}
        for r1, r2 in ((0, 3), (5, 1)):
            got[(r1, r2)] = pkg.parsexovs(eng, ts1, ts2, pkg.log_range(1.0, float(nsamp)), r1, r2)
        short = pkg.parsexovs(eng, ts1, ts2, pkg.log_range(1.0, float(nsamp)), 0, 3, nsamples=5)
        mats = {r: log.to_mat(r)[0] for r in (0, 1, 3, 5)}
    for (r1, r2), (mx2, sx2) in got.items():
        ref_m, ref_s = XR.parsexovs(mats[r1], mats[r2], ts1, ts2, list(pkg.log_range(1.0, float(nsamp))))
        assert len(ref_m) >= 4 and any(math.isnan(v) for v in ref_m) and sum(not math.isnan(v) for v in ref_m) >= 3
        _same_floats(mx2, ref_m)
        _same_floats(sx2, ref_s)
    ref_m, ref_s = XR.parsexovs(mats[0][:, :5], mats[3][:, :5], ts1[:5], ts2[:5], list(pkg.log_range(1.0, float(nsamp))))
    _same_floats(short[0], ref_m)
    _same_floats(short[1], ref_s)


def test_calls_do_not_disturb_a_resumed_run(pkg):
    seed, R, iters, step = 606, 7, 600, 100
    X = pkg.GraphRRG(30, 3, seed=seed)
    res = []
    for cut in (False, True):
        with pkg.Engine(X, R) as eng:
            eng.seed(seed)
            eng.init_spins_random()
            eng.snapshot_reserve(1)
            eng.snapshot_store(0)
            if not cut:
                Es, acc, staged = eng.rrr_mc(1.5, 2 * iters, step)
            else:
                Es1, acc1, st1 = eng.rrr_mc(1.5, iters, step)
                eng.set_resume(True)
                q = eng.cross_overlaps([-1, 0], [0, -1])
                h = eng.overlap_hist([-1, -1], [-1, 0])
                assert (q[0] == q[1].T).all() and int(h.sum()) == R * (R - 1) // 2 + R * (R - 1)
                Es2, acc2, st2 = eng.rrr_mc(1.5, iters, step)
                eng.set_resume(False)
                Es, acc, staged = np.concatenate([Es1, Es2], axis=1), acc1 + acc2, st1 + st2
            res.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config().s.copy()))
    for a, b in zip(*res):
        assert a.shape == b.shape and (a == b).all()


def _refused(pkg, eng, rc, *needles):
    assert rc == 1                                               # RRRMC_ERR_INVALID_ARG
    msg = pkg.lib().rrrmc_last_error(eng._ctx).decode()
    for n in needles:
        assert str(n) in msg, (n, msg)


def test_refusals(pkg):
    R = 70
    X = pkg.GraphRRG(130, 3, seed=3)
    L = pkg.lib()
    with pkg.Engine(X, R) as eng:
        eng.seed(3)
        eng.init_spins_random()
        eng.snapshot_reserve(3)
        eng.snapshot_store(0)
        eng.snapshot_store(1)                                    # slot 2 stays empty
        a, b = np.array([0, 1], np.int32), np.array([1, -1], np.int32)
        q = np.full(2 * R * R, 12345, np.int32)
        h = np.full(131, 12345, np.int64)
        ctx = eng._ctx
        # npairs = 0: fine, and nothing is written — NULL pointers included
        assert L.rrrmc_cross_overlaps(ctx, 0, None, None, 0, R, 0, R, None) == 0 and L.rrrmc_overlap_hist(ctx, 0, None, None, None) == 0
        assert L.rrrmc_cross_overlaps(ctx, 0, a, b, 0, R, 0, R, q) == 0 and L.rrrmc_overlap_hist(ctx, 0, a, b, h) == 0
        assert (q == 12345).all() and (h == 12345).all()
        _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, -1, a, b, 0, R, 0, R, q), "npairs", -1)
        _refused(pkg, eng, L.rrrmc_overlap_hist(ctx, -3, a, b, h), "npairs", -3)
        _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 2, None, b, 0, R, 0, R, q), "NULL")
        _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 2, a, None, 0, R, 0, R, q), "NULL")
        _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 2, a, b, 0, R, 0, R, None), "NULL", "q_out")
        _refused(pkg, eng, L.rrrmc_overlap_hist(ctx, 2, None, b, h), "NULL")
        _refused(pkg, eng, L.rrrmc_overlap_hist(ctx, 2, a, b, None), "NULL", "hist_out")
        for bad in (2, 3, -2):                                   # empty, beyond the reserved slots, below -1
            sl = np.array([1, bad], np.int32)
            _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 2, a, sl, 0, R, 0, R, q), "pair 1", "slot %d" % bad)
            _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 2, sl, b, 0, R, 0, R, q), "pair 1", "slot %d" % bad)
            _refused(pkg, eng, L.rrrmc_overlap_hist(ctx, 2, sl, b, h), "pair 1", "slot %d" % bad)
        for a0, nA in ((-1, 5), (0, 0), (0, -4), (66, 5), (70, 1), (0, 71)):
            _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 2, a, b, a0, nA, 0, R, q), "a0 = %d" % a0, "nA = %d" % nA)
            _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 2, a, b, 0, R, a0, nA, q), "b0 = %d" % a0, "nB = %d" % nA)
        with pytest.raises(pkg.RRRMCError, match="a0 = 69"):
            eng.cross_overlaps(0, 1, rowsA=(69, 2))
        with pytest.raises(pkg.RRRMCError, match="slot 2"):
            eng.overlap_hist(0, 2)
        with pytest.raises(ValueError):
            eng.cross_overlaps([0, 1], [0])
        # the caps, by the arguments alone: one pair too many, one matrix too many (2^26 / (70 * 70) = 13695.7)
        many = np.zeros(65536, np.int32)
        _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 65536, many, many, 0, 1, 0, 1, q), 65535, 65536)
        _refused(pkg, eng, L.rrrmc_overlap_hist(ctx, 65536, many, many, h), 65535, 65536)
        _refused(pkg, eng, L.rrrmc_cross_overlaps(ctx, 13696, many, many, 0, R, 0, R, q), 13696, 2 ** 26)
        assert (q == 12345).all() and (h == 12345).all()
        # at the caps the calls run: 65535 pairs of single rows, and the last matrix count that fits with small blocks
        ok = eng.cross_overlaps(many[:65535], many[:65535], rowsA=(3, 1), rowsB=(3, 1))
        assert ok.shape == (65535, 1, 1) and (ok == 130).all()
        assert eng.cross_overlaps(0, 1).shape == (1, R, R)       # and the context is as usable as before
