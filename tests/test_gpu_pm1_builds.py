"""Every build of the +-J standardMC kernels at every degree K = 1..7 and at its size limits, bit for bit against the oracle.

sweep_kernel<K, MODE 0..3>, plan_big / big_mask / big_apply / big_applyc / big_sweep and both colour-sweep builds are reached for every K,
on the smallest graph there is (the complete graph on K + 1 sites: one slot per level, N below a wavefront) and on a circulant graph of
about 200 sites; each case asserts, through Engine.sweep_layout(), that the kernels it asked for are the ones that ran.  No tolerances:
energies at every sample, accepted counts and final configurations of all replicas equal the oracle's, energy() and fields() of the
first and the last replica too.  Every case makes a second call that continues the streams at another beta (the threshold tables change
between the calls).  The matrix itself lives in tests/pm1_instances.py; tests/test_pm1_instances_cpu.py holds it to the full cross
products."""
import numpy as np
import pytest

import pm1_instances as PI

pytestmark = pytest.mark.gpu

R = PI.R
B1, B2 = PI.BETAS


def _setenv(monkeypatch, env):
    for name in PI.ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _numpy_graph(pkg, shape):
    A, J = PI.graph(shape)
    return pkg.GraphRRG.from_AJ(np.array(A), np.array(J))


def _resolve(v, C):
    return {"C": C, "C+1": C + 1}.get(v, v)


def _check_two_calls(pkg, oracle, X, seed, expect_path, calls, form="rrg", expect_lgr=None, R_=R):
    """calls(C) -> ((iters, step), (iters, step)) for the two calls, from the chunk length the context reports.  Returns the layout."""
    A, J = X.A, X.J.astype(np.int32)
    K = A.shape[1]
    with pkg.Engine(X, R_) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        lay0 = eng.sweep_layout()
        assert lay0[0] == -1 and lay0[1] == K and lay0[2] >= 64 and lay0[3] == -1          # no call yet
        (it1, st1), (it2, st2) = calls(lay0[2])
        C0 = eng.get_config()
        Es1, a1 = eng.standard_mc(B1, it1, st1)
        lay = eng.sweep_layout()
        Es2, a2 = eng.standard_mc(B2, it2, st2)
        assert eng.sweep_layout() == lay
        C2 = eng.get_config()
        E2 = eng.energy()
        lf = eng.fields()
    assert lay[0] == expect_path and lay[1] == K and lay[2] == lay0[2], (lay, expect_path)
    assert (lay[3] >= 0) == (4 <= expect_path <= 6)
    if expect_lgr is not None:
        assert lay[3] == expect_lgr
    r1 = oracle.standard_mc_sparse_batch(A, J, B1, it1, st1, seed, C0.s, form=form)
    r2 = oracle.standard_mc_sparse_batch(A, J, B2, it2, st2, seed, r1[1], it0=it1, form=form)
    assert Es1.shape == (R_, it1 // st1) == r1[0].shape and Es2.shape == (R_, it2 // st2) == r2[0].shape
    assert (Es1 == r1[0]).all() and (a1 == r1[2]).all()
    assert (Es2 == r2[0]).all() and (a2 == r2[2]).all()
    assert (C2.s == r2[1]).all()
    for r in (0, R_ - 1):
        e, lf_ref = oracle.sparse_energy(A, J, C2.s[r], want_fields=True)
        assert E2[r] == e and (lf[r] == lf_ref).all()
    if it1 >= 600:          # both verdicts are exercised: some moves accepted, some refused
        assert 0 < a1.min() and a1.max() < it1
    return lay


def _ragged_calls(C):
    """two chunks plus a ragged third, sampled at a step that divides neither the chunk nor the run; then a shorter call at another step"""
    it1, st1 = 2 * C + C // 2 + 3, 149
    it2, st2 = C + C // 3 + 1, 61
    assert it1 % st1 and C % st1 and it2 % st2 and C % st2
    return (it1, st1), (it2, st2)


# ---- (a) degree x path x shape -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,path,shape", PI.CASES_A)
def test_every_degree_on_every_path(pkg, oracle, monkeypatch, K, path, shape):
    env, expect = PI.PATHS[path]
    _setenv(monkeypatch, env)
    X = _numpy_graph(pkg, shape)
    _check_two_calls(pkg, oracle, X, 0xA000 + 64 * K + X.N, expect, _ragged_calls, expect_lgr=5 if expect >= 4 else None)


# ---- (b) long levels -----------------------------------------------------------------------------------------------------------------
# circulant(9000, K): a chunk's first level fills every row of a consumer batch.  The context's own layout at this size, as first observed
# on an MI355X (N > 8192 leaves MODE 2 and MODE 3; which one follows from the chunk lengths the 160 KiB of LDS allow):
NATURAL_9000 = {1: 2, 2: 2, 3: 2, 4: 2, 5: 2, 6: 2, 7: 3}          # (C = 1024, 1024, 1024, 640, 640, 640; K = 7: 896 in MODE 3)


@pytest.mark.parametrize("K,forced", PI.CASES_B)
def test_long_levels(pkg, oracle, monkeypatch, K, forced):
    _setenv(monkeypatch, {"RRRMC_FORCE_SINGLE": "1"} if forced else {})
    X = _numpy_graph(pkg, ("circulant", 9000, K))
    expect = 3 if forced else NATURAL_9000[K]

    def calls(C):
        return (3 * C + 5, 1009), (C + 11, 503)
    _check_two_calls(pkg, oracle, X, 0xB000 + K, expect, calls)


# ---- (c) replicas per workgroup x degree ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,lgr", PI.CASES_C)
def test_replicas_per_workgroup(pkg, oracle, monkeypatch, K, lgr):
    _setenv(monkeypatch, {"RRRMC_FORCE_BIG": "1", "RRRMC_BIG_LGR": str(lgr)})
    X = _numpy_graph(pkg, ("circulant", PI.n201(K), K))

    def calls(C):
        assert C == 4096
        return (2 * C + 809, 149), (C + 1367, 61)
    _check_two_calls(pkg, oracle, X, 0xC000 + 8 * K + lgr, PI.big_path(K, lgr), calls, expect_lgr=lgr)


def test_big_lgr_beyond_the_size_is_not_honoured(pkg, oracle, monkeypatch):
    """RRRMC_BIG_LGR asks for MORE replicas per workgroup than the image allows: the context keeps its own value (N = 40 000: r = 16)."""
    _setenv(monkeypatch, {"RRRMC_BIG_LGR": "5"})
    X = pkg.GraphRRG(40000, 3, seed=40)
    _check_two_calls(pkg, oracle, X, 0xC500, 5, lambda C: ((C + 7, 1000), (77, 10)), expect_lgr=4)


# ---- (d) the size limit, at natural size ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LD,no_masks", PI.CASES_D)
def test_size_limit(pkg, oracle, monkeypatch, LD, no_masks):
    """GraphEA(1024, 2): N = 2^20, the last size of the 20-bit site field, one replica per workgroup; GraphEA(80, 3): N = 512 000, two.
    The run must reach the top of the site field: an accepted move on a site whose highest bit of the field's range in use is set (>= 2^19
    at N = 2^20; at N = 512 000 < 2^19 no such site exists, there it is >= 2^18, beyond the largest N of any other test)."""
    _setenv(monkeypatch, {"RRRMC_BIG_NO_MASKS": no_masks})
    L_, D = LD
    seed = 0xD000 + L_
    X = pkg.GraphEA(L_, D, seed=seed)
    N = X.N
    lgr = {1 << 20: 0, 512000: 1}[N]
    top = 1 << 19 if N > (1 << 19) else 1 << 18
    A, J = X.A, X.J.astype(np.int32)
    it1, st1, it2, st2 = 2 * 4096 + 77, 1000, 4096 + 5, 999
    with pkg.Engine(X, 32) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        Es1, a1 = eng.standard_mc(B1, it1, st1)
        C1 = eng.get_config()
        E1 = eng.energy()
        lay = eng.sweep_layout()
        Es2, a2 = eng.standard_mc(B2, it2, st2)
        C2 = eng.get_config()
        E2 = eng.energy()
    assert lay == ((6 if no_masks == "1" else PI.big_path(2 * D, lgr)), 2 * D, 4096, lgr)
    for r in (0, 31):
        r1 = oracle.standard_mc_sparse(A, J, B1, it1, st1, seed, C0.s[r], replica=r, form="ea")
        assert (Es1[r] == r1[0]).all() and (C1.s[r] == r1[1]).all() and a1[r] == r1[2]
        assert E1[r] == oracle.sparse_energy(A, J, C1.s[r])
        r2 = oracle.standard_mc_sparse(A, J, B2, it2, st2, seed, r1[1], it0=it1, replica=r, form="ea")
        assert (Es2[r] == r2[0]).all() and (C2.s[r] == r2[1]).all() and a2[r] == r2[2]
        assert E2[r] == oracle.sparse_energy(A, J, C2.s[r])
        assert (C0.s[r, top // 64:] != C1.s[r, top // 64:]).any()          # the reach: a flip at a site >= top


def test_beyond_the_size_limit_is_refused(pkg, oracle, monkeypatch):
    """N > 2^20: standardMC answers RRRMC_ERR_UNSUPPORTED and names the colour sweeps; the context stays usable."""
    _setenv(monkeypatch, {})
    seed = 0xD401
    X = pkg.GraphEA(1025, 2, seed=seed)
    assert X.N > 1 << 20
    with pkg.Engine(X, 32) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        with pytest.raises(pkg.RRRMCError) as e:
            eng.standard_mc(B1, 100, 10)
        assert e.value.code == 3 and "beyond the random-site kernels" in str(e.value) and "rrrmc_colored_sweeps_async" in str(e.value)
        assert eng.sweep_layout()[0] == -1
        C0 = eng.get_config()
        E0 = eng.energy()
    assert (C0.s[0] == oracle.init_config(seed, 0, X.N)).all()
    assert E0[0] == oracle.sparse_energy(X.A, X.J.astype(np.int32), C0.s[0])


# ---- (e) colour sweeps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,counting,shape", PI.CASES_E)
def test_colour_sweeps_every_degree(pkg, oracle, monkeypatch, K, counting, shape):
    _setenv(monkeypatch, {})
    X = _numpy_graph(pkg, shape)
    A, J = X.A, X.J.astype(np.int32)
    color = np.arange(X.N, dtype=np.int32) if shape[0] == "complete" else oracle.greedy_coloring(A)
    seed = 0xE000 + 64 * K + X.N
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        eng.set_coloring(color)
        eng.colored_count_accepted(counting)
        C0 = eng.get_config()
        eng.colored_sweeps_async(B1, 12, 5)
        eng.sync()
        Es1, a1 = eng.fetch_results()
        lay = eng.sweep_layout()
        eng.colored_sweeps_async(B2, 3, 1)
        eng.sync()
        Es2, a2 = eng.fetch_results()
        C2 = eng.get_config()
        E2 = eng.energy()
        lf = eng.fields()
    assert lay[0] == (8 if counting else 7) and lay[1] == K and lay[3] == -1
    assert Es1.shape == (R, 2) and Es2.shape == (R, 3)
    for r in range(R):
        r1 = oracle.colored_sweeps_sparse(A, J, color, B1, 12, 5, seed, C0.s[r], replica=r)
        r2 = oracle.colored_sweeps_sparse(A, J, color, B2, 3, 1, seed, r1[1], sweep0=12, replica=r)
        assert (Es1[r] == r1[0]).all() and (Es2[r] == r2[0]).all() and (C2.s[r] == r2[1]).all()
        assert (a1[r], a2[r]) == ((r1[2], r2[2]) if counting else (-1, -1))
    for r in (0, R - 1):
        e, lf_ref = oracle.sparse_energy(A, J, C2.s[r], want_fields=True)
        assert E2[r] == e and (lf[r] == lf_ref).all()


# ---- (f) call shapes on every path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,call_shape", PI.CASES_F)
def test_call_shapes_on_every_path(pkg, oracle, monkeypatch, path, call_shape):
    env, expect = PI.PATHS[path]
    _setenv(monkeypatch, env)
    X = _numpy_graph(pkg, ("circulant", 200, 3))

    def calls(C):
        cs = (_resolve(call_shape[0], C), _resolve(call_shape[1], C))
        return cs, cs
    _check_two_calls(pkg, oracle, X, 0xF000 + 7 * PI.CALL_SHAPES.index(call_shape), expect, calls)
