"""The probes of tests/accept_boundary.py are what they claim to be (checked with the oracle's own functions and with mpmath), and the
shared det_exp / det_log1p — the same sequence of operations in the library (csrc/det_math.hpp) and in the oracle (oracle/philox_contract.h),
so a common error cancels in every parity test — are pinned to the true functions.  mpmath is required: without it these tests fail."""
import math

import numpy as np
import pytest

import accept_boundary as AB

DET_EXP_MAX_ULP = 2            # measured 1.09 at x = 91.842 (profiles/r15/accept_boundary.md); the next whole ulp
DET_EXP_MAX_SUB = 1            # ulps of the subnormal grid (measured 0.66)
DET_LOG1P_MAX_ULP = 3          # measured 2.31 at y = -0.20651 (2.8e-16 relative: the header's "~3e-16" holds); the next whole ulp


def _mp():
    import mpmath
    mpmath.mp.prec = 200
    return mpmath


def _ulps(got, true, mp):
    """|got - true| in units of the spacing of the doubles at the true value"""
    return float(abs(mp.mpf(got) - true) / mp.mpf(AB.ulp(float(true)) if float(true) != 0.0 else 2.0 ** -1074))


@pytest.mark.parametrize("key,t", [(k, t) for k in AB.PATHS for t in AB.classes_of(k)], ids=lambda v: str(v).replace(" ", ""))
def test_probes_are_live_and_sit_on_the_last_bits(oracle, key, t):
    mp = _mp()
    tg = AB.targets(oracle, key, t)
    assert len(tg) >= 3, "fewer than 3 live targets for %r, attempt %d after seeds 1..64" % (key, t)
    p = AB.path(oracle, key)
    for q in tg:
        assert q.t == t and 0 <= q.r < AB.PATHS[key] and q.dE > 0.0
        assert np.nextafter(q.beta_acc, math.inf) == q.beta_rej                       # adjacent doubles
        kw = p.make_run(q.seed, q.r)
        pa, pr = kw["run"](q.beta_acc, t - 1)[0], kw["run"](q.beta_rej, t - 1)[0]
        assert pa == pr == q.prefix                                                    # the same accepted count before attempt t
        assert kw["run"](q.beta_acc, t)[0] == pa + 1 and kw["run"](q.beta_rej, t)[0] == pr
        assert kw["run"](q.beta_acc, AB.iters_for(t))[0] != kw["run"](q.beta_rej, AB.iters_for(t))[0]      # visible in the GPU test's run
        assert q.u == oracle.rand53(q.seed, t, q.r) and q.site == oracle.site_of(q.seed, t, p.N)
        if p.energy is None:
            # dE is the sampler's own operand (the cached field): the verdicts are det_exp's, and u is within 2 ulps of the true exp(x)
            xa, xr = -q.beta_acc * q.dE, -q.beta_rej * q.dE
            assert q.u < oracle.det_exp(xa) and not q.u < oracle.det_exp(xr)
            # "exp(x) within 2 ulps of u" cannot be asked of both x once |x| > 1: xa and xr are adjacent-beta products, about one ulp of x
            # apart, and one ulp of x moves exp(x) by up to 2 |x| ulps (3.9 ulps at the probe x = -2.11 of GraphSKNormal(37), t = 2, whose
            # exp(xa) is 2.007 ulps above u).  What holds, and is asserted: u lies between the two true values, 2 ulps (det_exp's bound) allowed
            # on either side — for |x| < 1/2 that is the plain statement.
            ea, er = mp.exp(mp.mpf(xa)), mp.exp(mp.mpf(xr))
            one = mp.mpf(AB.ulp(q.u))
            assert er - 2 * one <= mp.mpf(q.u) <= ea + 2 * one
            if ea - er <= one:
                assert _ulps(q.u, ea, mp) <= 2.0 and _ulps(q.u, er, mp) <= 2.0
        else:
            # (the control has no field accessor: dE is E(flipped) - E, good to a few ulps of E — the verdict above is the sampler's own)
            assert abs(float(mp.exp(-mp.mpf(q.beta_acc) * mp.mpf(q.dE))) / q.u - 1.0) < 1e-9


def test_targets_are_reproducible(oracle):
    key = ("skn", 37)
    p = AB.path(oracle, key)
    for t in AB.CLASSES:
        assert AB.find_targets(oracle, p.make_run, p.N, t, AB.PATHS[key], iters=AB.iters_for(t)) == AB.targets(oracle, key, t)
    q = AB.targets(oracle, key, 33)[0]
    assert AB.four_betas(q)[1:3] == (q.beta_acc, q.beta_rej) and len(set(AB.four_betas(q))) == 4
    assert [AB.iters_for(t) for t in AB.CLASSES] == [128, 128, 128, 128, 192, 192]


@pytest.mark.parametrize("key", AB.LARGE_X_PATHS, ids=lambda v: str(v).replace(" ", ""))
def test_large_x_probes_hit_their_intervals(oracle, key):
    """one lane of the start block in each named interval of x: the estimate of spf_team_kernel denormal (-90) and zero (-110), both sides of the
    forced exponential at -700, a subnormal ldexp result (-722.6), both sides of the cut to 0 at -745.2; then x beyond any exponent and -inf"""
    seed, r, lane, site, rows = AB.large_x_case(oracle, key)
    assert 0 <= lane < 64 and site == oracle.site_of(seed, lane + 1, AB.path(oracle, key).N)
    assert [x for x, _, _ in rows] == list(AB.LARGE_X) + [None] * 3 and [b for _, b, _ in rows[-3:]] == list(AB.LARGE_BETA)
    for x, beta, xa in rows[:len(AB.LARGE_X)]:
        assert abs(xa - x) < 1e-9
    xs = [xa for _, _, xa in rows]
    assert -110 < xs[0] < -87 and -150 < xs[1] < -104                                  # 2^-126 = exp(-87.3), 2^-149 = exp(-103.3)
    assert -700 < xs[2] and xs[3] < -700 and -745.2 < xs[4] < -708.4 and -745.2 < xs[5] < -745 and xs[6] < -745.2
    e = [oracle.det_exp(x) for x in xs]
    assert 0 < e[4] < 2.0 ** -1022 and e[5] == 2.0 ** -1074 and e[6] == 0.0 and e[7] == e[8] == e[9] == 0.0
    assert xs[7] < -1e4 and xs[8] < -1e299 and xs[9] == -math.inf


def _exp_points():
    g = np.random.default_rng(20251020)
    xs = list(g.uniform(-745.0, 709.7, 40000))
    ln2 = math.log(2.0)
    for k in range(-1076, 1025):                                  # the seams of the reduction k = floor(x log2(e) + 1/2)
        c = (k + 0.5) * ln2
        if -745.2 <= c <= 709.7:
            lo, hi = np.nextafter(c, -math.inf), np.nextafter(c, math.inf)
            xs += [float(np.nextafter(lo, -math.inf)), float(lo), float(hi), float(np.nextafter(hi, math.inf))]
    return xs + [-745.2, -708.4, 709.7]


def test_det_exp_against_mpmath(oracle):
    mp = _mp()
    worst_n, worst_s = (0.0, None), (0.0, None)
    for x in _exp_points():
        true = mp.exp(mp.mpf(x))
        got = oracle.det_exp(x)
        if true >= mp.mpf(2) ** -1022:
            worst_n = max(worst_n, (_ulps(got, true, mp), x))
        else:
            worst_s = max(worst_s, (float(abs(mp.mpf(got) - true) / mp.mpf(2) ** -1074), x))
    print("det_exp: max error %.3f ulp at x = %r (normal results), %.3f ulp of the subnormal grid at x = %r" % (worst_n + worst_s))
    assert worst_n[0] <= DET_EXP_MAX_ULP, worst_n
    assert worst_s[0] <= DET_EXP_MAX_SUB, worst_s
    assert oracle.det_exp(-math.inf) == 0.0 and oracle.det_exp(0.0) == 1.0 and math.isnan(oracle.det_exp(math.nan))


def _log1p_points():
    g = np.random.default_rng(20251021)
    ys = [-float(u) for u in (g.integers(0, 1 << 53, 40000).astype(np.float64) * 2.0 ** -53)]      # y = -u, u a 53-bit uniform of [0, 1)
    ys += [-1.0 + k * 2.0 ** -53 for k in range(1, 2049)]                                           # the doubles next to -1
    ys += [-1.0 + float(v) for v in 2.0 ** g.uniform(-53, -1, 4000)]
    ys += [-float(v) for v in 2.0 ** g.uniform(-1074, -53, 4000)] + [-2.0 ** -53, -2.0 ** -54, -2.0 ** -1074, -0.0, 0.0]     # |y| < 2^-53
    ys += [-float(v) for v in 2.0 ** g.uniform(-53, 0, 8000)]                                       # every binade in between
    ys += [float(np.nextafter(c, d)) for c in (-1.0 + math.sqrt(0.5), -0.5, -0.25) for d in (-1.0, 0.0)] + [-0.5, -0.25]     # the seams of the reduction
    return [y for y in ys if -1.0 < y <= 0.0]


def test_det_log1p_against_mpmath(oracle):
    """the domain bklMC's rand_skip uses (src/DeltaE.jl:141-144): -1 < y <= 0"""
    mp = _mp()
    worst = (0.0, None)
    for y in _log1p_points():
        got = oracle.det_log1p(y)
        if y == 0.0:
            assert got == 0.0
            continue
        worst = max(worst, (_ulps(got, mp.log1p(mp.mpf(y)), mp), y))
    print("det_log1p: max error %.3f ulp at y = %r" % worst)
    assert worst[0] <= DET_LOG1P_MAX_ULP, worst
