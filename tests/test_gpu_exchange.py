"""GPU checks of the replica exchange between contexts (rrrmc_exchange_async / rrrmc_exchange_results, Engine.exchange, ParallelTempering;
DESIGN §4y) against the numpy restatement of tests/exchange_reference.py.  Every comparison is exact, except the two law tests, whose limit
is boltzmann_law's 1e-6 quantile."""
import math

import numpy as np
import pytest

import boltzmann_law as BL
import exchange_reference as XR

pytestmark = pytest.mark.gpu

CASE_R = [(c, R) for c in XR.PARITY_CASES for R in (c.R, 1)]
CASE_R_IDS = ["%s-R%d" % (c.id, R) for c, R in CASE_R]
INT_CASES = [c for c in XR.PARITY_CASES if c.id in ("rrg130-bitsliced", "rrglev20-rows")]


def _engine(pkg, X, R, seed, beta, iters, resume=False, debug=False, devices=None):
    e = pkg.Engine(X, R, devices=devices)
    if resume:
        e.set_resume(True)
    if debug:
        e.set_debug_checks(True)
    e.seed(seed)
    e.init_spins_random()
    Es = e.standard_mc(beta, iters, iters)[0]
    return e, Es


def _pair(pkg, case, R, **kw):
    X = case.make(pkg)
    a, Esa = _engine(pkg, X, R, case.seed_a, case.beta_a, case.iters, **kw)
    b, Esb = _engine(pkg, X, R, case.seed_b, case.beta_b, case.iters, **kw)
    return X, a, b, Esa, Esb


def _assert_tail_zero(X, s):
    if X.N % 64:
        assert not (s[:, -1] >> np.uint64(X.N % 64)).any(), "bits beyond N are set"


# ---- 1. parity per layout -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,R", CASE_R, ids=CASE_R_IDS)
def test_flags_energies_and_configurations_match_the_restatement(pkg, oracle, case, R):
    X, a, b, _, _ = _pair(pkg, case, R)
    with a, b:
        Ea0, Eb0 = np.asarray(a.energy(), np.float64), np.asarray(b.energy(), np.float64)
        ca, cb = a.get_config(), b.get_config()
        it_a = a.iterations_done()
        sw, Ea, Eb = a.exchange(b, case.beta_a, case.beta_b, case.xseed, case.rnd)
        fl = XR.flags(oracle, case.beta_a, case.beta_b, Ea0, Eb0, case.xseed, case.rnd)
        assert sw.dtype == bool and (sw == fl).all()
        assert (Ea == Ea0).all() and (Eb == Eb0).all()
        if R > 1:                                                # the last, partial word group holds both verdicts
            tail = fl[XR.tail_replicas(R)]
            assert tail.any() and not tail.all(), tail
        wa, wb = XR.swap_rows(ca.s, cb.s, fl)
        ga, gb = a.get_config(), b.get_config()
        assert (ga.s == wa).all() and (gb.s == wb).all()
        assert (ga.s[~fl] == ca.s[~fl]).all() and (gb.s[~fl] == cb.s[~fl]).all()          # unswapped replicas untouched
        _assert_tail_zero(X, ga.s)
        _assert_tail_zero(X, gb.s)
        assert a.iterations_done() == it_a
        # what the spins now hold is what energy() sees: the swapped energies
        assert (np.asarray(a.energy(), np.float64) == np.where(fl, Eb0, Ea0)).all()


@pytest.mark.parametrize("case", INT_CASES, ids=[c.id for c in INT_CASES])
def test_integer_models_take_the_tracked_energy(pkg, oracle, case):
    """no energy() call between the sampler and the exchange: the verdicts come from the energies standardMC tracked, which are exact — they
    equal energy() of a twin pair with the same history, and energy() of the swapped configurations afterwards"""
    X, a, b, Esa, Esb = _pair(pkg, case, case.R)
    _, ta, tb, _, _ = _pair(pkg, case, case.R)
    with a, b, ta, tb:
        Ea0, Eb0 = np.asarray(ta.energy(), np.float64), np.asarray(tb.energy(), np.float64)
        ca, cb = a.get_config(), b.get_config()
        assert ca == ta.get_config() and cb == tb.get_config()
        sw, Ea, Eb = a.exchange(b, case.beta_a, case.beta_b, case.xseed, case.rnd)
        assert (Ea == Ea0).all() and (Eb == Eb0).all()
        fl = XR.flags(oracle, case.beta_a, case.beta_b, Ea, Eb, case.xseed, case.rnd)
        assert (sw == fl).all()
        wa, wb = XR.swap_rows(ca.s, cb.s, fl)
        assert (a.get_config().s == wa).all() and (b.get_config().s == wb).all()
        for e in (a, b):                                         # no tracked energy describes the swapped spins
            with pytest.raises(pkg.RRRMCError) as ei:
                e.run_energy()
            assert ei.value.code == 2
        # the last call's samples belong to the temperature: still there
        assert (a.fetch_results()[0] == Esa).all() and (b.fetch_results()[0] == Esb).all()
        # a second exchange recomputes: its energies are the swapped ones
        sw2, Ea2, Eb2 = a.exchange(b, case.beta_a, case.beta_b, case.xseed, case.rnd + 1)
        assert (Ea2 == np.where(fl, Eb, Ea)).all() and (Eb2 == np.where(fl, Ea, Eb)).all()
        assert (sw2 == XR.flags(oracle, case.beta_a, case.beta_b, Ea2, Eb2, case.xseed, case.rnd + 1)).all()
        a.standard_mc(case.beta_a, 10, 10)
        a.run_energy()                                           # a sampling call has been made: tracked again


# ---- 2. forced verdicts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", XR.PARITY_CASES, ids=XR.PARITY_IDS)
def test_equal_betas_swap_every_replica(pkg, case):
    X, a, b, _, _ = _pair(pkg, case, case.R)
    with a, b:
        ca, cb = a.get_config(), b.get_config()
        sw, _, _ = a.exchange(b, 0.8, 0.8, 5, 0)
        assert sw.all()
        assert a.get_config() == cb and b.get_config() == ca


@pytest.mark.parametrize("case", [XR.PARITY_CASES[0], XR.PARITY_CASES[3]], ids=[XR.PARITY_IDS[0], XR.PARITY_IDS[3]])
def test_a_cold_and_a_hot_configuration_never_swap(pkg, oracle, case):
    X = case.make(pkg)
    a, _ = _engine(pkg, X, case.R, case.seed_a, 5.0, 200 * X.N)                  # a long cold run: near a ground state
    b = pkg.Engine(X, case.R)
    with a, b:
        b.seed(case.seed_b)
        b.init_spins_random()
        Ea0, Eb0 = np.asarray(a.energy(), np.float64), np.asarray(b.energy(), np.float64)
        ca, cb = a.get_config(), b.get_config()
        beta_a, beta_b = 20.0, 0.05
        xs = np.array([XR.x_of(beta_a, beta_b, ea, eb) for ea, eb in zip(Ea0, Eb0)])
        assert (xs < -745.2).all(), xs.max()                     # the condition: det_exp(x) = 0 everywhere
        sw, Ea, Eb = a.exchange(b, beta_a, beta_b, case.xseed, case.rnd)
        assert not sw.any() and (Ea == Ea0).all() and (Eb == Eb0).all()
        assert a.get_config() == ca and b.get_config() == cb


# ---- 3. the chain goes on correctly ---------------------------------------------------------------------------------------------------------
def _continues_like_a_twin(pkg, oracle, case, resume=False, debug=False, rrr=False):
    X, a, b, _, _ = _pair(pkg, case, case.R, resume=resume, debug=debug)
    with a, b:
        ca, cb = a.get_config(), b.get_config()
        sw, _, _ = a.exchange(b, case.beta_a, case.beta_b, case.xseed, case.rnd)
        assert sw.any() and not sw.all()
        wa, wb = XR.swap_rows(ca.s, cb.s, sw)
        for eng, seed, beta, want in ((a, case.seed_a, case.beta_a, wa), (b, case.seed_b, case.beta_b, wb)):
            twin, _ = _engine(pkg, X, case.R, seed, beta, case.iters, resume=resume, debug=debug)
            with twin:
                twin.set_config(pkg.Config(X.N, case.R, np.ascontiguousarray(want)))
                n = 3 * X.N + 7
                if rrr:
                    got, ref = eng.rrr_mc(beta, n, 5), twin.rrr_mc(beta, n, 5)
                else:
                    got, ref = eng.standard_mc(beta, n, 5), twin.standard_mc(beta, n, 5)
                for g, r in zip(got, ref):
                    assert g.dtype == r.dtype and (g == r).all()
                assert eng.get_config() == twin.get_config()
                if not rrr:
                    assert (np.asarray(eng.run_energy()) == np.asarray(twin.run_energy())).all()


@pytest.mark.parametrize("case", XR.PARITY_CASES, ids=XR.PARITY_IDS)
def test_next_standard_mc_equals_a_twin(pkg, oracle, case):
    _continues_like_a_twin(pkg, oracle, case)


@pytest.mark.parametrize("case", XR.PARITY_CASES, ids=XR.PARITY_IDS)
def test_next_standard_mc_equals_a_twin_under_resume(pkg, oracle, case):
    """a resumed call would continue from the tracked energy and the live caches: after an exchange it must start from energy(X, C)"""
    _continues_like_a_twin(pkg, oracle, case, resume=True)


DEBUG_CASES = [c for c in XR.PARITY_CASES if c.id in ("rrg130-bitsliced", "skn33-bytes", "rrgn130-lanes64")]     # the models the debug checks are wired for


@pytest.mark.parametrize("case", DEBUG_CASES, ids=[c.id for c in DEBUG_CASES])
def test_next_standard_mc_equals_a_twin_under_debug_checks(pkg, oracle, case):
    _continues_like_a_twin(pkg, oracle, case, debug=True)


def test_next_rrr_mc_starts_a_fresh_run(pkg, oracle):
    _continues_like_a_twin(pkg, oracle, XR.PARITY_CASES[0], resume=True, rrr=True)


# ---- 4. ordering without host syncs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [XR.PARITY_CASES[0], XR.PARITY_CASES[2], XR.PARITY_CASES[3]], ids=[XR.PARITY_IDS[0], XR.PARITY_IDS[2], XR.PARITY_IDS[3]])
def test_queued_sequence_equals_the_synchronised_one(pkg, case):
    X = case.make(pkg)
    betas, n = (1.0, 0.8, 0.6), 4 * X.N

    def sequence(sync_every):
        engs = [pkg.Engine(X, case.R) for _ in betas]
        try:
            for t, e in enumerate(engs):
                e.seed(case.seed_a + t)
                e.init_spins_random()

            def step(f):
                f()
                if sync_every:
                    for e in engs:
                        e.sync()
            for t, e in enumerate(engs):
                step(lambda: e.standard_mc_async(betas[t], n, n))
            step(lambda: engs[0].exchange(engs[1], betas[0], betas[1], case.xseed, 0, wait=False))
            step(lambda: engs[1].exchange(engs[2], betas[1], betas[2], case.xseed, 1, wait=False))
            for t, e in enumerate(engs):
                step(lambda: e.standard_mc_async(betas[t], n, n))
            for e in engs:
                e.sync()
            return ([e.get_config().s.copy() for e in engs], [e.fetch_results() for e in engs],
                    [engs[0].exchange_results(), engs[1].exchange_results()])
        finally:
            for e in engs:
                e.close()

    qc, qr, qx = sequence(False)
    sc, sr, sx = sequence(True)
    for t in range(3):
        assert (qc[t] == sc[t]).all()
        assert (qr[t][0] == sr[t][0]).all() and (qr[t][1] == sr[t][1]).all()
    for k in range(2):
        for g, r in zip(qx[k], sx[k]):
            assert (g == r).all()
        assert qx[k][0].any()                                   # the exchanges did move configurations


# ---- 5. two-shard contexts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [XR.PARITY_CASES[0], XR.PARITY_CASES[3], XR.PARITY_CASES[1]], ids=[XR.PARITY_IDS[0], XR.PARITY_IDS[3], XR.PARITY_IDS[1]])
def test_two_shards_equal_one_device(pkg, case):
    R = 70
    out = []
    for devices in (None, [0, 0]):
        X, a, b, _, _ = _pair(pkg, case, R, devices=devices)
        with a, b:
            res = a.exchange(b, case.beta_a, case.beta_b, case.xseed, case.rnd)
            out.append((res, a.get_config().s.copy(), b.get_config().s.copy(), a.standard_mc(case.beta_a, 50, 50), b.standard_mc(case.beta_b, 50, 50)))
    (r1, a1, b1, sa1, sb1), (r2, a2, b2, sa2, sb2) = out
    for g, r in zip(r1, r2):
        assert (g == r).all()
    assert r1[0].any() and not r1[0].all()
    assert (a1 == a2).all() and (b1 == b2).all()
    for g, r in zip(sa1 + sb1, sa2 + sb2):
        assert (g == r).all()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def _config_or_none(pkg, e):
    if e is None:
        return None
    try:
        return e.get_config()
    except pkg.RRRMCError:                                       # no configuration yet
        return None


def _refused(pkg, a, b, code, word, beta_a=0.9, beta_b=0.6):
    before = [_config_or_none(pkg, a), _config_or_none(pkg, b)]
    with pytest.raises(pkg.RRRMCError) as ei:
        if b is None:
            pkg._lib.check(pkg.lib().rrrmc_exchange_async(a._ctx, None, beta_a, beta_b, 1, 0), a._ctx)
        else:
            a.exchange(b, beta_a, beta_b, 1, 0)
    assert ei.value.code == code, str(ei.value)
    assert word in str(ei.value), str(ei.value)
    for e, c in zip((a, b), before):
        if c is not None:
            assert e.get_config() == c
    with pytest.raises(pkg.RRRMCError) as ei:                   # and no exchange has been recorded
        a.exchange_results()
    assert ei.value.code == 2


def _ready(pkg, X, R, seed=3, **kw):
    e = pkg.Engine(X, R, **kw)
    e.seed(seed)
    e.init_spins_random()
    return e


def test_refusals(pkg):
    X = pkg.GraphRRG(40, 3, seed=5)
    assert pkg.lib().rrrmc_exchange_async(None, None, 0.5, 0.6, 1, 0) == 1
    assert pkg.lib().rrrmc_exchange_results(None, None, None, None, None) == 1
    with _ready(pkg, X, 33) as a, _ready(pkg, X, 33, seed=4) as b:
        _refused(pkg, a, None, 1, "NULL")
        _refused(pkg, a, a, 1, "same")
        for ba, bb in ((math.inf, 0.5), (0.5, -math.inf), (math.nan, 0.5), (0.5, math.nan)):
            _refused(pkg, a, b, 1, "finite", ba, bb)
        with pkg.Engine(X, 33) as nospins:                       # a graph but no configuration
            _refused(pkg, a, nospins, 2, "configuration")
            _refused(pkg, nospins, a, 2, "configuration")
        # a context that was never given a graph: only the C ABI makes one
        import ctypes
        raw = ctypes.c_void_p()
        pkg._lib.check(pkg.lib().rrrmc_ctx_create(ctypes.byref(raw), X.model_kind, X.N, X.K, 33, 0, 0))
        try:
            ca = a.get_config()
            for first, second in ((a._ctx, raw), (raw, a._ctx)):
                rc = pkg.lib().rrrmc_exchange_async(first, second, 0.9, 0.6, 1, 0)
                msg = pkg.lib().rrrmc_last_error(first).decode()
                assert rc == 2 and "graph" in msg and "configuration" not in msg, (rc, msg)
            assert a.get_config() == ca
            assert pkg.lib().rrrmc_exchange_results(raw, None, None, None, None) == 2
        finally:
            pkg.lib().rrrmc_ctx_destroy(raw)
        with _ready(pkg, X, 34) as c:
            _refused(pkg, a, c, 2, "differ")
        with _ready(pkg, X, 33, replica0=64) as c:
            _refused(pkg, a, c, 2, "differ")
        with _ready(pkg, pkg.GraphRRG(42, 3, seed=5), 33) as c:
            _refused(pkg, a, c, 2, "differ")
        with _ready(pkg, pkg.GraphRRG(40, 4, seed=5), 33) as c:
            _refused(pkg, a, c, 2, "differ")
        with _ready(pkg, pkg.GraphRRGNormal(40, 3, seed=5), 33) as c:
            _refused(pkg, a, c, 2, "differ")
        with _ready(pkg, X, 33, devices=[0, 0]) as m:            # one device against a device list
            _refused(pkg, a, m, 3, "device list")
            _refused(pkg, m, a, 3, "device list")
        with _ready(pkg, X, 96, devices=[0, 0]) as m2, _ready(pkg, X, 96, devices=[0, 0, 0]) as m3:
            _refused(pkg, m2, m3, 3, "device lists")
        # a refusal leaves a working pair: the exchange still runs
        Ea0, Eb0 = a.energy(), b.energy()
        sw, Ea, Eb = a.exchange(b, 0.9, 0.6, 1, 0)
        assert sw.shape == (33,) and (Ea == Ea0).all() and (Eb == Eb0).all()


UNSUPPORTED = [
    ("GraphQuant", lambda pkg: pkg.GraphQuant(pkg.GraphRRG(10, 3, seed=5), 4, 0.5, 2.0)),
    ("GraphRobustEnsemble", lambda pkg: pkg.Graph0RE(5, 3, 0.6, 1.2)),
    ("GraphLocalEntropy", lambda pkg: pkg.Graph0LE(5, 3, 0.6, 1.2)),
    ("Discretized", lambda pkg: pkg.GraphRRGNormalDiscretized(10, 3, (-1, 0, 1), seed=5)),
    ("GraphPercStep", lambda pkg: pkg.GraphPercStep(21, 10, seed=5)),
    ("GraphSAT", lambda pkg: pkg.GraphSAT(20, 3, 4.0, seed=5)),
    ("GraphPSpin3", lambda pkg: pkg.GraphPSpin3(12, 3, seed=5)),
    ("GraphTopologicalLocalEntropy", lambda pkg: pkg.Graph0TLE(5, 3, 0.6, 0.3, 1.2)),
    ("GraphAddFields", lambda pkg: pkg.GraphAddFields(np.linspace(-1.0, 1.0, 21), pkg.GraphSK(21, seed=5))),
    ("GraphAddSubFields", lambda pkg: pkg.GraphAddSubFields(np.linspace(-1.0, 1.0, 21), pkg.GraphSKNormal(21, seed=5))),
    ("GraphAddFields", lambda pkg: pkg.GraphAddFields(np.linspace(-1.0, 1.0, 12), pkg.GraphPSpin3(12, 3, seed=5))),      # a wrapper, not the 3-spin graph
    ("GraphMixed", lambda pkg: pkg.GraphMixed(pkg.GraphSK(21, seed=5), pkg.GraphPercStep(21, 10, seed=5))),
    ("GraphMixed", lambda pkg: pkg.GraphAddFields(np.linspace(-1.0, 1.0, 21), pkg.GraphMixed(pkg.GraphSK(21, seed=5), pkg.GraphPercStep(21, 10, seed=5)))),
    ("GraphCommStep", lambda pkg: pkg.GraphCommStep(3, 7, 10, seed=6)),
    ("GraphCommStep", lambda pkg: pkg.GraphCommReLU(2, 4, 5, seed=6)),            # the committee machines share one name list
    ("GraphPercXEntr", lambda pkg: pkg.GraphPercXEntr(21, 10, 1.0, seed=5)),
    ("GraphPercStep", lambda pkg: pkg.GraphPercLinear(21, 10, seed=5)),
]


@pytest.mark.parametrize("name,make", UNSUPPORTED, ids=["%s-%d" % (u[0], k) for k, u in enumerate(UNSUPPORTED)])
def test_other_models_are_refused_by_name(pkg, name, make):
    X = make(pkg)
    with _ready(pkg, X, 4) as a, _ready(pkg, X, 4, seed=4) as b:
        _refused(pkg, a, b, 3, name)


# ---- 7. the Boltzmann law on the device -------------------------------------------------------------------------------------------------
LAW_BETAS = (0.4, 0.7, 1.0)


@pytest.mark.parametrize("name", ["GraphRRG-10", "GraphRRGNormal-8"])
def test_parallel_tempering_follows_the_law_at_every_beta(pkg, name):
    X = pkg.GraphRRG(10, 3, seed=11) if name == "GraphRRG-10" else pkg.GraphRRGNormal(8, 3, seed=5)
    E = BL.exact_energies(X)
    with pkg.ParallelTempering(X, LAW_BETAS, R=65536, seed=20251) as pt:
        assert pt.run(100, 4) == 100
        print(name, "acceptance", pt.accept_rate, "round trips", int(pt.round_trips.sum()))
        idx = [BL._state_index(pt.config(t), X.N) for t in range(pt.T)]
    for t, beta in enumerate(LAW_BETAS):
        counts = np.bincount(idx[t], minlength=len(E))
        other = LAW_BETAS[t + 1] if t + 1 < len(LAW_BETAS) else LAW_BETAS[t - 1]
        v = BL.Verdict(BL.score(counts, BL.boltzmann(E, beta)), BL.score(counts, BL.boltzmann(E, other)))
        print("%s beta %.1f: chi2 %.0f (limit %.0f, %d dof, pooled mass %.4f); against beta %.1f: chi2 %.0f (limit %.0f)"
              % (name, beta, v.law.chi2, v.law.limit, v.law.dof, v.law.pooled_mass, other, v.power.chi2, v.power.limit))
        BL.assert_verdict(v)


# ---- 8. the driver's bookkeeping -----------------------------------------------------------------------------------------------------------
def test_driver_bookkeeping(pkg, oracle):
    """labels, flags, acceptance, round trips and energies of a run, recomputed from what the run recorded.  energies[round][t] is the energy
    of temperature t after the round's sampling and before its swaps.  A standardMC sample precedes the move of its iteration
    (src/RRRMC.jl:104-108), so the round's last sample is the energy one move EARLIER and equals it only when that move was rejected: the
    check is therefore made against energy() of the configurations the round left (exact: the swapped energies), and the last sample is
    held to differ from it by one move's dE at most."""
    X = pkg.GraphRRG(10, 3, seed=11)
    betas, R, rounds = (0.2, 0.5, 0.8, 1.1), 70, 40
    after, last = [], []

    def hook(rd, pt):
        last.append(np.stack([pt.engine(t).fetch_results()[0][:, -1] for t in range(pt.T)]))          # still there after the exchange
        after.append(np.stack([np.asarray(pt.engine(t).energy(), np.float64) for t in range(pt.T)]))
        return rd < rounds - 3                                   # the hook's False stops the run

    with pkg.ParallelTempering(X, betas, R=R, seed=99) as pt:
        assert pt.run(rounds, 6, hook=hook) == rounds - 2 and pt.round == rounds - 2
        labels = np.repeat(np.arange(pt.T)[:, None], R, axis=1)
        acc, att = np.zeros(pt.T - 1), np.zeros(pt.T - 1)
        for rd in range(pt.round):
            assert (pt.attempted[rd] == np.array([(t - rd) % 2 == 0 for t in range(pt.T - 1)])).all()
            assert not pt.swaps[rd][~pt.attempted[rd]].any()
            E = pt.energies[rd]
            assert E.shape == (pt.T, R) and np.isin(E - last[rd], (0, 2, -2, 6, -6)).all()
            want = E.copy()                                      # the energies the contexts hold after the round's swaps
            for t in np.flatnonzero(pt.attempted[rd]):
                fl = XR.flags(oracle, betas[t], betas[t + 1], E[t], E[t + 1], 99, rd)
                assert (pt.swaps[rd][t] == fl).all()
                s = pt.swaps[rd][t]
                want[t][s], want[t + 1][s] = E[t + 1][s], E[t][s]
                labels[t][s], labels[t + 1][s] = labels[t + 1][s].copy(), labels[t][s].copy()
                acc[t] += s.sum()
                att[t] += R
            assert (after[rd] == want).all()
        assert (pt.labels == labels).all()
        assert (np.sort(pt.labels, axis=0) == np.arange(pt.T)[:, None]).all()          # a permutation per ladder
        assert (pt.accept_rate == acc / att).all() and (acc > 0).all()
        # round trips from the recorded swaps alone: follow every walker, count bottom -> top -> bottom per ladder
        trips = np.zeros(R, np.int64)
        for r in range(R):
            pos = list(range(pt.T))                              # pos[w]: where the walker that started at w is
            phase = [1 if w == 0 else 0 for w in range(pt.T)]
            for rd in range(pt.round):
                for t in np.flatnonzero(pt.attempted[rd]):
                    if pt.swaps[rd][t][r]:
                        wa, wb = pos.index(t), pos.index(t + 1)
                        pos[wa], pos[wb] = t + 1, t
                top, bot = pos.index(pt.T - 1), pos.index(0)
                if phase[top] == 1:
                    phase[top] = 2
                if phase[bot] == 2:
                    trips[r] += 1
                phase[bot] = 1
        assert (pt.round_trips == trips).all()
        print("round trips", int(trips.sum()), "acceptance", pt.accept_rate)
        assert pt.overlap_hist(0).sum() == R * (R - 1) // 2
        assert pt.engine(1).R == R and pt.config(3).R == R
