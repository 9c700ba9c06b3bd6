"""GPU parity for the three ensembles over sparse Float64 slices — GraphEARE, GraphEALE, GraphEATLE (src/REAliases.jl:43-75,
src/LEAliases.jl:43-75, src/TLEAliases.jl:36-68) and the generic constructors over a GraphRRGNormal: rrrMC(X::DoubleGraph) and standardMC
through the HIP kernels equal the plain-Python restatement (tests/sparse_slice_reference.py inside re_reference / le_reference /
tle_reference) bit for bit — energies at every sample, final configuration, accepted and staged counts, the DeltaECache's classes and set
sizes, tracked and fresh energy(X, C), the per-slice energies, cenergy and distances.

Shapes: EA(L=2, D=2) (every bond doubled, uA shorter than the row, odd M), EA(3, 2) (even M), EA(3, 3) with 70 chains (K = 6, more chains
than a wavefront, unaligned) and a GraphRRGNormal(10, 3).  Every case runs two calls, fresh and resumed; the LDS build and the forced global
build are compared with each other and with the reference.

The sampler's β and the graphs' γ are such that the chain takes both branches and rejects direct moves (the slices' move_last path): the
reference run counts them and the test asserts it — with staged_thr = 0.5 at least one rejected direct move AND one staged iteration, with
staged_thr = 0.0 (every iteration direct) a rejected direct move, with staged_thr = 1.0 (every iteration staged) a staged iteration."""
import os

import numpy as np
import pytest

import le_reference as LE
import re_reference as RE
import sparse_slice_reference as SP
import tle_reference as TLE

pytestmark = pytest.mark.gpu

GAMMA, LAM, BETA_G, BETA = 1.2, 0.4, 1.5, 0.6
# name -> (L, D) of an EA lattice or ("rrg", N, K); M; R; the replicas of the batch that are checked
SHAPES = {
    "ea_2_2": ((2, 2), 3, 2, [0, 1]),
    "ea_3_2": ((3, 2), 4, 3, [0, 1, 2]),
    "ea_3_3": ((3, 3), 5, 70, [0, 1, 69]),
    "rrg_10_3": (("rrg", 10, 3), 4, 2, [0, 1]),
}
FAMILIES = {
    "re": dict(run=RE.RrrRun, std=RE.standard_mc, rows=lambda M: M, env="RRRMC_RE_NO_LDS"),
    "le": dict(run=LE.RrrRun, std=LE.standard_mc, rows=lambda M: M + 1, env="RRRMC_LE_NO_LDS"),
    "tle": dict(run=TLE.RrrRun, std=TLE.standard_mc, rows=lambda M: M + 1, env="RRRMC_TLE_NO_LDS"),
}


def _graph(pkg, fam, shape, M, seed):
    """(the device graph, a factory of fresh reference graphs)"""
    if shape[0] == "rrg":
        G = pkg.GraphRRGNormal(shape[1], shape[2], seed=seed)
        X = (pkg.GraphRobustEnsemble(G.N, M, GAMMA, BETA_G, G) if fam == "re" else pkg.GraphLocalEntropy(G.N, M, GAMMA, BETA_G, G) if fam == "le"
             else pkg.GraphTopologicalLocalEntropy(G.N, M, GAMMA, LAM, BETA_G, G))
    else:
        L, D = shape
        X = (pkg.GraphEARE(L, D, M, GAMMA, BETA_G, seed=seed) if fam == "re" else pkg.GraphEALE(L, D, M, GAMMA, BETA_G, seed=seed) if fam == "le"
             else pkg.GraphEATLE(L, D, M, GAMMA, LAM, BETA_G, seed=seed))
    A, J = X.X1.A, X.X1.J
    ref = ((lambda: SP.make_re(A, J, M, GAMMA, BETA_G)) if fam == "re" else (lambda: SP.make_le(A, J, M, GAMMA, BETA_G)) if fam == "le"
           else (lambda: SP.make_tle(A, J, M, GAMMA, LAM, BETA_G)))
    return X, ref


def _counted(run):
    """count apply_move calls: a direct iteration makes one, and a second one when the move is rejected (the undo)"""
    run.n_apply = 0
    inner = run.apply_move

    def apply_move(move):
        run.n_apply += 1
        return inner(move)
    run.apply_move = apply_move
    return run


def _cache(eng, fam):
    return eng.tle_cache() if fam == "tle" else eng.rrr_cache()


def _check_observables(eng, fam, R, A, J, M, finals):
    if fam == "re":
        Es = eng.re_energies()
        for r, s in finals:
            assert np.asarray(Es if R == 1 else Es[r]).tolist() == SP.re_energies(A, J, M, s)
        return
    Es, Ec, D = eng.le_energies(), eng.cenergy(), eng.distances()
    for r, s in finals:
        assert np.asarray(Es if R == 1 else Es[r]).tolist() == SP.le_energies(A, J, M, s)
        assert float(Ec if R == 1 else Ec[r]) == SP.cenergy(A, J, M, s)
        assert np.asarray(D if R == 1 else D[r]).tolist() == LE.distances(len(A), M, s)


def _check_rrr(pkg, oracle, fam, shape_name, thr, iters=2500, step=250, calls=2, resume=False, devices=None, debug=False, check_reps=None):
    shape, M, R, reps = SHAPES[shape_name]
    reps = reps if check_reps is None else check_reps
    F = FAMILIES[fam]
    seed = 8330017 + 31 * M + sum(ord(c) for c in shape_name)
    X, ref = _graph(pkg, fam, shape, M, seed)
    A, J = X.X1.A, X.X1.J
    N = X.Nk * F["rows"](M)
    assert X.N == N
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
            Es, acc, staged = eng.rrr_mc(BETA, iters, step, staged_thr=thr)
            outs.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config(), _cache(eng, fam), eng.run_energy()))
        if resume:
            eng.set_resume(False)
        Ef = eng.energy()
        finals = []
        rejected_direct = staged_total = 0
        for r in reps:
            s = RE.config_from_chunks(C0.s[r], N)
            assert (C0.s[r] == oracle.init_config(seed, r, N)).all()
            assert E0[r] == ref().energy(s.copy())
            run = None
            for c in range(calls):
                if run is None or not resume:          # a resumed call continues the run; otherwise a call starts like a reference call
                    run = _counted(F["run"](ref(), s, BETA, seed, oracle, replica=r, it0=c * iters, staged_thr=thr))
                    acc0 = st0 = 0
                else:
                    acc0, st0 = run.accepted, run.staged_its
                it0, ap0 = run.it, run.n_apply
                es = run.run(iters, step)
                rejected_direct += (run.n_apply - ap0) - ((run.it - it0) - (run.staged_its - st0))
                staged_total += run.staged_its - st0
                Es, acc, staged, C1, (pos, sizes), Etr = outs[c]
                assert np.asarray(Es[r]).tolist() == [float(e) for e in es], (r, c)
                assert acc[r] == run.accepted - acc0 and staged[r] == run.staged_its - st0, (r, c)
                assert (C1.s[r] == RE.chunks_from_config(s)).all(), (r, c)
                p_ref, sz_ref = run.cache_view()
                assert (np.asarray(pos[r]).astype(np.int64) == p_ref.astype(np.int64)).all() and (sizes[r] == sz_ref).all(), (r, c)
                assert Etr[r] == run.E, (r, c)
            assert Ef[r] == ref().energy(s.copy())
            finals.append((r, s))
        _check_observables(eng, fam, R, A, J, M, finals)
    if reps:
        # the case proves something only if the slices' undo path (a rejected direct move) and the staged branch were taken
        if thr < 1.0:
            assert rejected_direct >= 1, "no rejected direct move in the reference run"
        if thr > 0.0:
            assert staged_total >= 1, "no staged iteration in the reference run"
    return outs


@pytest.mark.parametrize("resume", [False, True], ids=["fresh", "resumed"])
@pytest.mark.parametrize("thr", [0.5, 0.0, 1.0])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_rrr_parity(pkg, oracle, fam, shape, thr, resume):
    _check_rrr(pkg, oracle, fam, shape, thr, resume=resume)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_standard_parity_fresh_then_resumed(pkg, oracle, fam, shape):
    shp, M, R, reps = SHAPES[shape]
    F = FAMILIES[fam]
    seed = 6110023 + 31 * M + sum(ord(c) for c in shape)
    X, ref = _graph(pkg, fam, shp, M, seed)
    A, J = X.X1.A, X.X1.J
    N = X.N
    iters, step = 3000, 100
    with pkg.Engine(X, R) as eng:
        eng.seed(seed)
        eng.init_spins_random()
        C0 = eng.get_config()
        out1 = eng.standard_mc(BETA, iters, step)
        out1 = (out1[0].copy(), out1[1].copy(), eng.get_config(), eng.run_energy())
        eng.set_resume(True)
        out2 = eng.standard_mc(BETA, iters, step)
        out2 = (out2[0].copy(), out2[1].copy(), eng.get_config(), eng.run_energy())
        eng.set_resume(False)
        finals = []
        for r in reps:
            s = RE.config_from_chunks(C0.s[r], N)
            Xr = ref()
            E = None
            for c, (Es, acc, C1, Etr) in enumerate((out1, out2)):
                es, E, a = F["std"](Xr, s, BETA, iters, step, seed, oracle, replica=r, it0=c * iters, E=E)
                assert Es[r].tolist() == [float(e) for e in es] and acc[r] == a, (r, c)
                assert (C1.s[r] == RE.chunks_from_config(s)).all(), (r, c)
                assert Etr[r] == E, (r, c)
                assert 0 < a < iters                     # accepted moves (update_cache!) and rejected ones both happen
            finals.append((r, s))
        _check_observables(eng, fam, R, A, J, M, finals)


class _forced_build:
    """RRRMC_<FAM>_NO_LDS=1 (lds = False) or RRRMC_<FAM>_LDS=1 (lds = True) for the block, the other switch unset.  The first forces the
    thread-per-chain build (RE, LE) or the wavefront build with all its arrays in global memory (TLE); the second forces the one-wavefront-
    per-chain LDS build whenever the chain's own arrays fit.  Only the TLE reports which build ran (Engine.tle_build); nothing introspects
    the RE / LE build, so their LDS leg relies on the switch that forces it."""

    def __init__(self, fam, lds):
        self.no_lds, self.want = FAMILIES[fam]["env"], FAMILIES[fam]["env"].replace("_NO_LDS", "_LDS")
        self.set = {self.want: "1"} if lds else {self.no_lds: "1"}

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in (self.no_lds, self.want)}
        os.environ.update(self.set)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("shape", ["ea_2_2", "ea_3_3"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_lds_and_global_builds_agree_with_each_other_and_the_reference(pkg, oracle, fam, shape):
    res = []
    for lds in (False, True):
        with _forced_build(fam, lds):
            outs = _check_rrr(pkg, oracle, fam, shape, 0.5, resume=True)
            if fam == "tle":
                X, _ = _graph(pkg, fam, SHAPES[shape][0], SHAPES[shape][1], 1)
                with pkg.Engine(X, 2) as eng:
                    eng.seed(3)
                    eng.init_spins_random()
                    eng.rrr_mc(BETA, 200, 100)
                    assert eng.tle_build() == (1 if lds else 2)
            res.append(outs)
    a, b = res
    for (Ea, aa, sa, Ca, (pa, za), Ta), (Eb, ab, sb, Cb, (pb, zb), Tb) in zip(a, b):
        assert Ea.tolist() == Eb.tolist() and (aa == ab).all() and (sa == sb).all() and (Ca.s == Cb.s).all()
        assert (pa == pb).all() and (za == zb).all() and (Ta == Tb).all()


@pytest.mark.parametrize("fam,M", [("re", 5), ("le", 5), ("tle", 3)])
def test_lds_build_whose_slice_state_stays_in_global_memory(pkg, fam, M):
    """EA(64, 2): Nk = 4096, K = 4.  The chain's own arrays fit the 160 KiB of a workgroup (RE, M = 5: 69 KiB; LE, M = 5: 81 KiB; TLE, M = 3:
    about 137 KiB) and the slices' fields on top of them do not (8 rows (Nk + K + 1) bytes = 160 / 192 / 128 KiB more), so the LDS build runs
    with lfields, the undo record and move_last left in global memory.  Two resumed calls, bit for bit against the build that keeps
    everything in global memory."""
    X, _ = _graph(pkg, fam, (64, 2), M, 4242)
    rows = FAMILIES[fam]["rows"](M)
    N, Nk, W = X.N, X.Nk, 2 * ((X.N + 63) // 64)
    # the LDS bytes of the chain's own arrays, as re_rrr_lds_bytes / le_rrr_lds_bytes / tle_rrr_lds_bytes (csrc) size them
    if fam == "tle":
        L2 = 2 * len(X.tables())
        base = 2048 + 12 * L2 + 4 * N + 4 * W + 2 * (2 * N) + Nk
    else:
        base = 4 * W + 2 * N + N + Nk + (128 if fam == "re" else 136) + 2048
    assert Nk == 4096 and base <= 160 * 1024 < base + 8 * rows * (Nk + X.K + 1) + 4 * rows
    res = []
    for lds in (False, True):
        with _forced_build(fam, lds), pkg.Engine(X, 3) as eng:
            eng.seed(77)
            eng.init_spins_random()
            eng.set_resume(True)
            out = []
            for _ in range(2):
                Es, acc, staged = eng.rrr_mc(BETA, 700, 100)
                out.append((Es.copy(), acc.copy(), staged.copy(), eng.get_config().s.copy(), _cache(eng, fam), eng.run_energy().copy()))
            if fam == "tle":
                assert eng.tle_build() == (1 if lds else 2)
            eng.set_resume(False)
            out.append(eng.energy().copy())
            res.append(out)
    a, b = res
    for (Ea, aa, sa, ca, (pa, za), Ta), (Eb, ab, sb, cb, (pb, zb), Tb) in zip(a[:2], b[:2]):
        assert Ea.tolist() == Eb.tolist() and (aa == ab).all() and (sa == sb).all() and (ca == cb).all()
        assert (pa == pb).all() and (za == zb).all() and (Ta == Tb).all()
        assert 0 < aa.min() and aa.max() < 700          # accepted and rejected moves: the slices' update and its undo both ran
    assert (a[2] == b[2]).all()


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_two_device_context_equals_one_device(pkg, oracle, fam):
    a = _check_rrr(pkg, oracle, fam, "ea_3_3", 0.5, iters=1500, step=100, calls=1, check_reps=[0, 69], devices=[0, 0])
    b = _check_rrr(pkg, oracle, fam, "ea_3_3", 0.5, iters=1500, step=100, calls=1, check_reps=[])
    assert a[0][0].tolist() == b[0][0].tolist() and (a[0][3].s == b[0][3].s).all()
    assert (a[0][4][0] == b[0][4][0]).all() and (a[0][4][1] == b[0][4][1]).all()


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_debug_switch_passes(pkg, oracle, fam):
    _check_rrr(pkg, oracle, fam, "ea_2_2", 0.5, debug=True)
    X, _ = _graph(pkg, fam, (3, 2), 4, 77)
    with pkg.Engine(X, 3) as eng:
        eng.set_debug_checks(True)
        eng.seed(5)
        eng.init_spins_random()
        eng.rrr_mc(BETA, 3000, 100)
        eng.rrr_mc(BETA, 3000, 100, staged_thr=1.0)
        eng.standard_mc(BETA, 3000, 100)
        eng.sync()
        Etr, E = eng.run_energy(), eng.energy()
        assert (np.abs(Etr - E) <= 1e-10 * np.maximum(1.0, np.abs(E))).all()
