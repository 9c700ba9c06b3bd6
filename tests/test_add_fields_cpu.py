"""GraphAddFields / GraphAddSubFields without a GPU: the model table (rrrmc.jl_amd/csrc/af_models.hpp, compiled on its own with the
sanitizers on), the plain-Python restatement (tests/add_fields_reference.py) held to the reference's own energy assertion, to g's own
standardMC chain and to the exact Boltzmann law, and what the creator and the front end refuse before any device is asked for."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import add_fields_reference as AF
import boltzmann_law as BL
import perc_reference as PR
import re_reference as RE
import sat_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY, SK, SKN, PERC_STEP, PERC_LINEAR, COMM_STEP, COMM_RELU, SAT, COMM_QU = 0, 1, 2, 3, 4, 5, 6, 8, 9      # enum rrrmc_re_slice
KINDS = [EMPTY, SK, SKN, PERC_STEP, PERC_LINEAR, COMM_STEP, COMM_RELU, SAT, COMM_QU]
ADD, ADDSUB = 1, 2


# ---- the family's table -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    assert shutil.which("g++") is not None, "the table's stand-alone check needs g++"
    exe = str(tmp_path_factory.mktemp("af_models") / "af_models_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "af_models_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    by_model, by_pair = {}, {}
    for f in (l.split() for l in out.stdout.splitlines()):
        if f[0] == "M":
            by_model[int(f[1])] = (int(f[2]), int(f[3]), int(f[4]))
        else:
            by_pair[(int(f[1]), int(f[2]))] = int(f[3])
    return by_model, by_pair


def test_the_18_models_from_48_upward_and_no_other(table):
    by_model, by_pair = table
    want = {48 + n: (ADD, s) for n, s in enumerate(KINDS)}
    want.update({57 + n: (ADDSUB, s) for n, s in enumerate(KINDS)})
    assert len(want) == 18 and sorted(want) == list(range(48, 66))
    for model in range(100):
        fam, s, ms = by_model[model]
        assert (fam, s) == want.get(model, (0, -1)), model
        if model in want:
            assert ms == s
    assert by_model[99] == (0, -1, -1) and by_model[34][2] == SAT and by_model[33][2] == -1      # unknown; an ensemble's slice; a stand-alone graph
    for (fam, s), model in by_pair.items():
        assert model == ({v: k for k, v in want.items()}.get((fam, s), 0))


def test_the_header_names_the_same_numbers():
    import re
    with open(os.path.join(ROOT, "include", "rrrmc_hip.h"), encoding="utf-8") as fh:
        enum = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"RRRMC_MODEL_(AS?F_[A-Z_]+) = (\d+)", fh.read()))
    names = ["EMPTY", "SK", "SKN", "PERC_STEP", "PERC_LINEAR", "COMM_STEP", "COMM_RELU", "SAT", "COMM_QU"]
    assert enum == dict([("AF_" + n, 48 + k) for k, n in enumerate(names)] + [("ASF_" + n, 57 + k) for k, n in enumerate(names)])


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def _sat(oracle, N=33, seed=1033):
    A, J = SR.gen_ksat(oracle, N, 3, 4.2, seed)
    return N, A, J


def _fields(N, seed=11):
    h = np.random.default_rng(seed).normal(size=N)
    h[0], h[N // 2], h[N - 1] = 0.0, -0.0, 0.0
    return h


@pytest.mark.parametrize("sub", [False, True], ids=["AddFields", "AddSubFields"])
@pytest.mark.parametrize("kind", ["sat", "skn"])
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.5], ids=["direct", "default", "staged"])
def test_tracked_energy_and_weights_along_a_walk(oracle, kind, sub, thr):
    """the reference's own assertion (RRRMC.jl:250): |E - energy(X, C)| < 1e-10 at every iteration, on a fresh graph object; and the
    sampler's weights are prior(β ΔE_i) of the configuration"""
    beta = 0.9
    if kind == "sat":
        N, A, J = _sat(oracle)
        mk = lambda: SR.SatRef(N, A, J)
    else:
        N = 24
        Jm = np.random.default_rng(3).normal(size=(N, N)) / np.sqrt(N)
        Jm = np.triu(Jm, 1)
        Jm = Jm + Jm.T
        mk = lambda: RE.SliceSKN(Jm)
    h = _fields(N)
    s = np.random.default_rng(5).integers(0, 2, N).astype(np.int64)
    run = AF.AfRun(AF.AddFields(h, mk(), sub), s, beta, 4242, oracle, staged_thr=thr)
    worst = [0.0]

    def after(r):
        fresh = AF.AddFields(h, mk(), sub).energy(s.copy())
        worst[0] = max(worst[0], abs(r.E - fresh))
        assert abs(r.E - fresh) < 1e-10
        for i in range(N):
            d = r.X.delta0(s, i)
            assert r.dEs[i] == d and r.ds.v[i] == r.prior(beta * d)
    run.run(400, 1, after=after)
    assert run.accepted > 20 and run.ds.refreshes >= 1
    assert run.staged_its == (0 if thr == 0.0 else 400 if thr == 1.5 else run.staged_its)


@pytest.mark.parametrize("wrapper", ["AddSubFields", "AddFields-zeros"])
@pytest.mark.parametrize("kind", ["sat", "perc"])
def test_standard_mc_is_the_chain_of_g(oracle, kind, wrapper):
    """standardMC on GraphAddSubFields(h, g), and on GraphAddFields(zeros, g), is the standardMC chain of g's own restatement"""
    beta, iters, step, seed = 1.1, 1500, 50, 777
    if kind == "sat":
        N, A, J = _sat(oracle)
        mk = lambda: SR.SatRef(N, A, J)
        own = lambda s: SR.standard_mc(SR.ClauseCache(N, A, J), s, beta, iters, step, seed, oracle, replica=3)
    else:
        N = 21
        xi = np.random.default_rng(8).integers(0, 2, (12, N))
        mk = lambda: PR.make(xi, False)
        own = lambda s: PR.standard_mc(PR.make(xi, False), s, beta, iters, step, seed, oracle, replica=3)
    h = _fields(N) if wrapper == "AddSubFields" else np.zeros(N)
    s0 = np.random.default_rng(6).integers(0, 2, N).astype(np.int64)
    sa, sb = s0.copy(), s0.copy()
    Es, E, acc = AF.standard_mc(AF.AddFields(h, mk(), wrapper == "AddSubFields"), sa, beta, iters, step, seed, oracle, replica=3)
    es, e, a = own(sb)
    assert [float(x) for x in es] == Es and float(e) == E and a == acc and acc > 50
    assert (sa == sb).all()


# ---- the Boltzmann law on 9 spins -------------------------------------------------------------------------------------------------------
BL_ITERS, BL_BETA, BL_SEED = 250, 0.9, 9301          # the GPU twin (tests/test_gpu_add_fields_boltzmann.py) runs the same iterations
BL_CPU_R, BL_CPU_POWER = 1792, 1.5          # with these, the pooled tail of each law (β and 1.5 β, both wrappers) expects at least 5 chains


def bl_instance():
    """the fields of the 9-spin instance (over GraphSAT(9, 3, 20 / 9; seed 1): 20 three-literal clauses), on a grid of 1/2 so that the
    energies of GraphAddFields fall on few exact levels and every ΔE is exact in Float64"""
    return np.array([0.5, -0.5, 0.0, 1.0, -1.0, 0.5, 0.0, -0.5, 1.0])


def violated(A, J, sg):
    up = sg > 0
    E = np.zeros(len(sg), np.float64)
    for Aa, Ja in zip(A, J):
        sat = np.zeros(len(sg), bool)
        for i, j in zip(Aa, Ja):
            sat |= up[:, i] == bool(j)
        E += ~sat
    return E


@pytest.mark.parametrize("sub", [False, True], ids=["AddFields", "AddSubFields"])
def test_the_restatement_follows_the_boltzmann_law(oracle, sub):
    """rrrMC on GraphAddSubFields follows exp(-β E_g) whatever the fields; on GraphAddFields it follows exp(-β (Σ h σ + E_g))"""
    A, J = SR.gen_ksat(oracle, 9, 3, 20 / 9, 1)
    h = bl_instance()
    sg = 2 * BL.enumerate_states(9) - 1
    E = violated(A, J, sg) + (0.0 if sub else sg @ h)
    case = BL._case("rrr-%s-9" % ("GraphAddSubFields" if sub else "GraphAddFields"), None, "rrr", BL_BETA, BL_ITERS, BL_SEED, R=BL_CPU_R, observable="energy")
    rng = np.random.default_rng(77)
    last = np.zeros(BL_CPU_R)
    for r in range(BL_CPU_R):
        s = rng.integers(0, 2, 9).astype(np.int64)
        run = AF.AfRun(AF.AddFields(h, SR.SatRef(9, A, J), sub), s, BL_BETA, BL_SEED, oracle, replica=r)
        run.run(BL_ITERS, BL_ITERS)
        last[r] = run.E
        assert abs(run.E - (SR.pure_energy(A, J, s) + (0.0 if sub else float((2 * s - 1) @ h)))) < 1e-10
    v = BL.judge(case, E, None, last, power=BL_CPU_POWER)
    print("chi2 %s: law %.1f (limit %.1f, %d dof), at %.1f beta %.1f (limit %.1f)" % (case.id, v.law.chi2, v.law.limit, v.law.dof, BL_CPU_POWER, v.power.chi2, v.power.limit))
    BL.assert_verdict(v)


# ---- refusals before any device query ---------------------------------------------------------------------------------------------------
def _create(pkg, null_out=False, kind=SAT, sub=0, N=33, K2=0, R=4, device=0, replica0=0):
    lib = pkg.lib()
    ctx = C.c_void_p()
    f = C.CDLL(lib._name).rrrmc_ctx_create_af
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_uint32]
    rc = f(None if null_out else C.byref(ctx), kind, sub, N, K2, R, device, replica0)
    msg = lib.rrrmc_last_error(None)
    assert ctx.value is None
    return int(rc), (msg.decode() if msg else "")


def test_the_creator_refuses_by_name_before_any_device_query(pkg):
    cases = [
        (dict(null_out=True), 1, "out is NULL"),
        (dict(kind=7), 1, "slice_kind must be"), (dict(kind=-1), 1, "GraphAddFields"), (dict(kind=10), 1, "slice_kind must be"),
        (dict(sub=2), 1, "sub must be 0"), (dict(sub=-1), 1, "sub must be 0"),
        (dict(N=0), 1, "N and R must be >= 1"), (dict(R=0), 1, "N and R must be >= 1"),
        (dict(kind=PERC_STEP, N=20), 1, "N must be odd"), (dict(kind=PERC_LINEAR, N=32769), 3, "perceptron kernels"),
        (dict(kind=COMM_STEP, N=21, K2=0), 1, "K2"), (dict(kind=COMM_STEP, N=22, K2=7), 1, "K2"),
        (dict(kind=COMM_STEP, N=28, K2=7), 1, "K1 must be odd"), (dict(kind=COMM_RELU, N=21, K2=7), 1, "must be even"),
        (dict(kind=COMM_QU, N=30, K2=6), 1, "K1 must be even"), (dict(kind=COMM_QU, N=182 * 182, K2=182), 3, "committee machine kernels"),
        (dict(kind=SAT, N=65536), 3, "K-SAT kernels"), (dict(kind=EMPTY, N=65536), 3, "GraphAddFields kernels"),
        (dict(kind=SKN, N=65536), 3, "GraphAddFields kernels"),
        (dict(replica0=16), 1, "replica0 must be a multiple of 32"), (dict(replica0=33), 1, "replica0"),
    ]
    for kw, code, word in cases:
        rc, msg = _create(pkg, **kw)
        assert rc == code and word in msg, (kw, rc, msg)
        assert "no HIP device" not in msg and "out of range (0.." not in msg
    for sub in (0, 1):          # the multi-device creator hands the same refusals on
        lib = pkg.lib()
        ctx = C.c_void_p()
        rc = lib.rrrmc_ctx_create_multi(C.byref(ctx), (57 if sub else 48) + 3, 20, 0, 0, 4, np.zeros(1, np.int32), 1, 0)
        assert rc == 1 and b"N must be odd" in lib.rrrmc_last_error(None) and ctx.value is None


def test_set_fields_without_a_context_and_the_front_end(pkg):
    assert pkg.lib().rrrmc_af_set_fields(None, np.zeros(4)) == 1
    h = np.zeros(21)
    h[5] = np.nan
    with pytest.raises(ValueError, match="finite"):
        pkg.GraphAddFields(h, pkg.GraphPercStep(21, 12))
    with pytest.raises(ValueError, match="finite"):
        pkg.GraphAddSubFields(np.full(21, np.inf), pkg.GraphPercStep(21, 12))
    with pytest.raises(TypeError, match="sparse graphs"):
        pkg.GraphAddFields(np.zeros(16), pkg.GraphRRG(16, 3))
    with pytest.raises(TypeError, match="GraphQuant and the ensembles"):
        pkg.GraphAddSubFields(np.zeros(9), pkg.Graph0RE(3, 3, 0.5, 1.0))
    with pytest.raises(ValueError, match="incompatible length, fields size=5 graph size=21"):
        pkg.GraphAddFields(np.zeros(5), pkg.GraphPercStep(21, 12))
    X = pkg.GraphAddSubFields(np.zeros(24), pkg.GraphCommQu(4, 6, 10))
    assert (X.model_kind, X.slice_kind, X.K2, X._multi_args()) == (65, 9, 6, (65, 24, 6, 0))
    assert pkg.GraphAddFields(np.zeros(7)).model_kind == 48 and pkg.GraphAddFields(np.zeros(9), pkg.GraphSAT(9, 3, 2.0)).model_kind == 55
