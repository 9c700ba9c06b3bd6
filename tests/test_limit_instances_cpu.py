"""tests/limit_instances.py held to its claims without a GPU: every entry sits on the bound it names, its reference run decides something
(some replica accepts some but not all of its attempts; the perceptron's p / m boundary sets change), the LDS byte counts written beside the
boundary pairs are what the host's formulas give and lie on both sides of the limit, the crafted perceptrons reach both ends of an int16
and have the energy of the definition, and the GPU test is parametrised over the whole table."""
import math
import re
import os

import numpy as np
import pytest

import limit_instances as LI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    """the value of ``constexpr <type> name = <integer> | <integer> * <integer> | <integer> << <integer>;``: declared exactly once in the
    kernels' sources, and in no other form"""
    found = []
    for f in sorted(os.listdir(os.path.join(ROOT, "rrrmc.jl_amd", "csrc"))):
        src = open(os.path.join(ROOT, "rrrmc.jl_amd", "csrc", f)).read()
        found += re.findall(r"\bconstexpr\s+(?:long long|int64_t|int)\s+%s\s*=\s*([^;]+);" % re.escape(name), src)
    assert len(found) == 1, (name, found)
    m = re.fullmatch(r"(\d+)(?:ll)?(?:\s*(\*|<<)\s*(\d+))?", found[0].strip())
    assert m, (name, found[0])
    a = int(m.group(1))
    return a if m.group(2) is None else a * int(m.group(3)) if m.group(2) == "*" else a << int(m.group(3))


def test_the_literal_bounds_are_the_headers():
    assert LI.PERC_N[1] == 32767 == _header_constant("kPercNmax")
    assert LI.PERC_P[1] == 4096 == _header_constant("kPercPmax")
    assert LI.AF_N[1] == 65535 == _header_constant("kAfNmax")
    assert LI.KLDS_LIMIT == 163840 == _header_constant("kLdsLimit")
    assert _header_constant("kReMmax") == 32 and _header_constant("kLeMmax") == 31
    assert _header_constant("kSatNmax") == 65535 and _header_constant("kSatDegMax") == 65535 and _header_constant("kSatLenMax") == 8
    assert _header_constant("kSatMcMax") == 1 << 20
    for e in LI.ENTRIES:
        for what, lit, const in e.bounds:
            if re.fullmatch(r"k\w+", const):
                assert lit == _header_constant(const), (e.name, what)


@pytest.mark.parametrize("name", LI.NAMES)
def test_entry_sits_on_its_bound(pkg, name):
    e = LI.BY_NAME[name]
    X = LI.graph(pkg, name)
    sp = e.spec
    have = {"N": X.N, "P": getattr(X, "P", None) or getattr(getattr(X, "X1", None), "P", None), "M": getattr(X, "M", None)}
    if e.family == "sat":
        have.update({"max occurrences": X.max_conn, "literals": X.K, "clauses": X.M, "largest variable id": int(X._vars.max())})
    if e.family == "comm":
        have["K2"] = X.K2
    if e.family == "xentr":
        have["table entries"] = len(X.Hs)
    if e.family == "af":
        have["tree levels"] = math.ceil(math.log2(X.N))
    if e.lds is not None:
        fn = {"re": lambda: LI.re_comm_lds_bytes(sp["Nk"], sp["M"], sp["K2"], 64) if sp["slice"] == "comm" else
              LI.re_lds_bytes(sp["Nk"], sp["M"], (sp["P"] + 63) // 64 if sp["slice"] == "perc" else 0),
              "le": lambda: LI.le_lds_bytes(sp["Nk"], sp["M"], (sp["P"] + 63) // 64 if sp["slice"] == "perc" else 0), "af": lambda: LI.af_lds_bytes(sp["N"]),
              "quant": lambda: LI.quant_qu_std_lds_bytes(sp["K1"] * sp["K2"], sp["M"], sp["K2"], 64) if sp.get("qu") else
              LI.quant_std_lds_bytes(sp["Nk"], sp["M"], (sp["P"] + 63) // 64)}[e.family]
        have["LDS bytes"] = fn()
        assert e.lds == have["LDS bytes"]
        if e.build is not None and e.family == "quant":
            assert e.build == (2 if e.lds <= LI.KLDS_LIMIT else 1)             # rrrmc_quant_pattern_build: 2 staged in LDS, 1 not
        elif e.build is not None:
            assert e.build == (LI.LDS if e.lds <= LI.KLDS_LIMIT else LI.GLOBAL)
    assert e.bounds
    for what, lit, const in e.bounds:
        if what in have:
            assert have[what] == lit, (name, what, have[what], lit)
    if "crafted" in sp:
        c, xi = LI.crafted_patterns(sp["N"], sp["crafted"], sp["seed"])
        d = LI.perc_deltas(xi.astype(np.int64), c)
        assert d.max() == 32767 and d.min() == -32767
        assert sorted(np.unique(d).tolist()) == ([-32767, 1, 32767] if sp["crafted"][2] else [-32767, 32767])
        assert [(d == 32767).sum(), (d == -32767).sum(), (d == 1).sum()] == list(sp["crafted"])
        for w in range(64):                   # both ends in every mask word
            assert {32767, -32767} <= set(d[64 * w:64 * w + 64].tolist())
    assert 1 <= e.run["R"] <= 3 and 300 <= e.run["iters"] <= 2000 and e.run["iters"] % e.run["step"] == 0


def test_boundary_pairs_are_adjacent_and_straddle_the_limit():
    assert len(LI.PAIRS) == 9 and len(LI.XENTR_PAIRS) == 2 and len(LI.SPF_PAIRS) == 2
    for a, b in LI.PAIRS:
        ea, eb = LI.BY_NAME[a], LI.BY_NAME[b]
        assert ea.lds <= LI.KLDS_LIMIT < eb.lds and not ea.env and not eb.env
        assert (ea.build, eb.build) == ((2, 1) if ea.family == "quant" else (LI.LDS, LI.GLOBAL))
        sa, sb = ea.spec, eb.spec
        diff = {k: (sa[k], sb[k]) for k in sa if sa[k] != sb[k]}
        assert len(diff) == 1 and list(diff.values())[0][1] - list(diff.values())[0][0] == 1, diff         # N + 1, Nk + 1 or M + 1
        assert ea.run == eb.run
    # the rules are monotone in the parameter: nothing above the first shape fits, everything below it does
    assert all(LI.af_lds_bytes(N) <= LI.KLDS_LIMIT for N in range(1, 4097)) and all(LI.af_lds_bytes(N) > LI.KLDS_LIMIT for N in range(4097, 65536, 7))
    assert all((LI.re_lds_bytes(Nk, 3) <= LI.KLDS_LIMIT) == (Nk <= 15581) for Nk in range(15000, 16000))
    assert all((LI.le_lds_bytes(Nk, 3) <= LI.KLDS_LIMIT) == (Nk <= 11974) for Nk in range(11500, 12500))
    assert all((LI.re_lds_bytes(3, M, 64) <= LI.KLDS_LIMIT) == (M <= 17) for M in range(3, 33))
    assert all((LI.le_lds_bytes(3, M, 64) <= LI.KLDS_LIMIT) == (M <= 16) for M in range(3, 32))
    assert all((LI.quant_std_lds_bytes(3, M, 64) <= LI.KLDS_LIMIT) == (M <= 17) for M in range(3, 33))
    assert all((LI.quant_qu_std_lds_bytes(4, M, 2, 64) <= LI.KLDS_LIMIT) == (M <= 4) for M in range(3, 33))
    assert all((LI.re_comm_lds_bytes(9, M, 3, 64) <= LI.KLDS_LIMIT) == (M <= 4) for M in range(3, 33))
    # GraphPercXEntr's table: (N + 1) 8 in the thread build; PW 64 (8 + 2) + (N + 1) 8 + 4 W in the wave build (PW = 2); N odd, the next is N + 2
    wave = lambda N: 2 * 64 * 10 + (N + 1) * 8 + 4 * 2 * ((N + 63) // 64)          # noqa: E731
    want = {"xentr_thread_N20479_P65_pair": (20480 * 8, 163840), "xentr_thread_N20481_P65_pair": (20482 * 8, 163856),
            "xentr_wave_N20005_P65_pair": (wave(20005), 163832), "xentr_wave_N20007_P65_pair": (wave(20007), 163848)}
    for ens, (a, b) in zip(("re", "le"), LI.SPF_PAIRS):
        ea, eb = LI.BY_NAME[a], LI.BY_NAME[b]
        assert eb.spec["L"] - ea.spec["L"] == 1 and ea.run == eb.run and not ea.env and not eb.env and ea.build == eb.build == LI.LDS
        ba, bb = (LI.spf_lds_bytes(ens, x.spec["L"], 3) for x in (ea, eb))
        assert (ba, bb) == (ea.bounds[0][1], eb.bounds[0][1]) and ba <= LI.KLDS_LIMIT < bb
        own = LI.re_lds_bytes if ens == "re" else LI.le_lds_bytes
        assert own(eb.spec["Nk"], 3) <= LI.KLDS_LIMIT                      # the chain's own arrays fit on both sides: the LDS build runs
    for a, b in LI.XENTR_PAIRS:
        ea, eb = LI.BY_NAME[a], LI.BY_NAME[b]
        assert eb.spec["N"] - ea.spec["N"] == 2 and ea.run == eb.run and ea.env == eb.env and ea.build == eb.build
        for e in (ea, eb):
            assert e.bounds[0][1] == want[e.name][0] == want[e.name][1]
        assert ea.bounds[0][1] <= LI.KLDS_LIMIT < eb.bounds[0][1]


@pytest.mark.parametrize("name", LI.NAMES)
def test_reference_run_decides_something(pkg, oracle, name):
    e = LI.BY_NAME[name]
    ref = LI.reference(pkg, oracle, name)
    iters = e.run["iters"]
    assert len(ref) == e.run["R"]
    for c in range(2):
        if LI.rejection_free(e):              # zero residual: every proposal is accepted; the energies still move with the chosen sites
            assert all(r["calls"][c]["acc"] in (iters - 1, iters) for r in ref)       # (one draw on a weight of 0 refreshes the tree instead)
            assert all(len(set(r["calls"][c]["Es"])) > 1 for r in ref)
        else:
            assert any(0 < r["calls"][c]["acc"] < iters for r in ref), [r["calls"][c]["acc"] for r in ref]
    for r in ref:
        assert len(r["calls"][0]["Es"]) == iters // e.run["step"]
    if e.family == "comm":
        # the committee machines' boundary sets ({Δ2 = ±1}, {Δ2 = 2}, {Δ2 = 0}; CommQu: the misclassified set) differ between start and end
        assert all(r["members"][0] != r["members"][2] for r in ref), name
    if e.family == "perc":
        # the p / m boundary sets differ between start and end: in every replica, except at N = 1 or 3, where a chain has 2 or 8 states and
        # may come back to where it started (there: some replica)
        assert (all if e.spec["N"] > 3 else any)(r["members"][0] != r["members"][2] for r in ref), name
    if e.run["sampler"].startswith("rrr"):
        st = [r["calls"][c]["staged"] for r in ref for c in range(2)]
        if e.run["thr"] == 0.0:
            assert st == [0] * len(st)
        elif e.run["thr"] == 1.5:
            assert st == [iters] * len(st)
        else:
            assert all(0 <= x <= iters for x in st)


@pytest.mark.parametrize("shape", ["ragged", (10, 3, 4.2), (33, 5, 8.0)], ids=str)
def test_vectorised_sat_reference_is_the_plain_one(pkg, oracle, shape):
    """SatVec against sat_reference.ClauseCache at small shapes: same energies, same ΔE at every site, same trajectory"""
    import sat_reference as SR
    X = pkg.GraphSAT.from_clauses(*SR.ragged_instance()) if shape == "ragged" else pkg.GraphSAT(*shape, seed=1000 + shape[0])
    rng = np.random.default_rng(3)
    for r in range(3):
        s = rng.integers(0, 2, X.N).astype(np.int64)
        s2 = s.copy()
        plain, vec = SR.ClauseCache(X.N, X.A, X.J), LI.SatVec(X)
        assert plain.energy(s) == vec.energy(s2) == SR.pure_energy(X.A, X.J, s)
        assert [plain.delta_energy(i) for i in range(X.N)] == [vec.delta_energy(i) for i in range(X.N)] == [SR.pure_delta(X.A, X.J, X.T, s, i) for i in range(X.N)]
        for beta, it0 in ((0.0, 0), (1.5, 400)):
            a = SR.standard_mc(plain, s, beta, 400, 20, 77, oracle, replica=r, it0=it0, E=plain.energy(s))
            b = SR.standard_mc(vec, s2, beta, 400, 20, 77, oracle, replica=r, it0=it0, E=vec.energy(s2))
            assert a == b and (s == s2).all() and 0 < a[2]
            assert [plain.delta_energy(i) for i in range(X.N)] == [vec.delta_energy(i) for i in range(X.N)]


@pytest.mark.parametrize("relu,K1,K2,P", [(False, 3, 7, 10), (False, 5, 3, 70), (True, 4, 6, 10), (True, 2, 4, 129)])
def test_vectorised_committee_reference_is_the_plain_one(pkg, oracle, relu, K1, K2, P):
    """CommVec against comm_reference's CommStepRef / CommReLURef at small shapes: same energies, same ΔE at every site, same trajectory"""
    import comm_reference as CR
    X = (pkg.GraphCommReLU if relu else pkg.GraphCommStep)(K1, K2, P, seed=6)
    xi, y = X.patterns(), X.labels()
    rng = np.random.default_rng(4)
    for r in range(3):
        s = rng.integers(0, 2, X.N).astype(np.int64)
        s2 = s.copy()
        plain, vec = CR.make(K2, xi, y), LI.CommVec(K2, xi, y)
        assert plain.energy(s) == vec.energy(s2) == CR.energy_from_definition(K2, xi, y, s)
        assert [plain.delta(s, i) for i in range(X.N)] == [vec.delta(s2, i) for i in range(X.N)]
        for beta, it0 in ((0.0, 0), (0.8, 400)):
            a = CR.standard_mc(plain, s, beta, 400, 20, 78, oracle, replica=r, it0=it0, E=plain.energy(s))
            b = CR.standard_mc(vec, s2, beta, 400, 20, 78, oracle, replica=r, it0=it0, E=vec.energy(s2))
            assert a == b and (s == s2).all() and 0 < a[2]
            assert [plain.delta(s, i) for i in range(X.N)] == [vec.delta(s2, i) for i in range(X.N)]
            assert vec.d1.T.tolist() == [list(col) for col in zip(*plain.d1)] and vec.d2.tolist() == plain.d2


@pytest.mark.parametrize("K1,K2,P", [(4, 6, 10), (2, 4, 129), (6, 2, 70)])
def test_vectorised_commqu_reference_is_the_plain_one(pkg, oracle, K1, K2, P):
    """CommQuVec against comm_qu_reference.CommQuRef at small shapes: same energies, same ΔE at every site, same trajectory"""
    import comm_qu_reference as CQ
    X = pkg.GraphCommQu(K1, K2, P, seed=6)
    xi, y = X.patterns(), X.labels()
    rng = np.random.default_rng(5)
    for r in range(3):
        s = rng.integers(0, 2, X.N).astype(np.int64)
        s2 = s.copy()
        plain, vec = CQ.make(K2, xi, y), LI.CommQuVec(K2, xi, y)
        assert plain.energy(s) == vec.energy(s2)
        assert [plain.delta(s, i) for i in range(X.N)] == [vec.delta(s2, i) for i in range(X.N)]
        for beta, it0 in ((0.0, 0), (0.8, 400)):
            a = CQ.standard_mc(plain, s, beta, 400, 20, 79, oracle, replica=r, it0=it0, E=plain.energy(s))
            b = CQ.standard_mc(vec, s2, beta, 400, 20, 79, oracle, replica=r, it0=it0, E=vec.energy(s2))
            assert a == b and (s == s2).all() and 0 < a[2]
            assert [plain.delta(s, i) for i in range(X.N)] == [vec.delta(s2, i) for i in range(X.N)]
            assert vec.d2.tolist() == plain.d2


def test_crafted_commqu_sits_on_both_ends(pkg, oracle):
    e = LI.BY_NAME["commqu_crafted_delta2_ends"]
    c, xi, y = LI.crafted_qu(e.spec["K1"], e.spec["P"], e.spec["seed"])
    V = LI.CommQuVec(2, xi, y)
    V.energy(c.astype(np.int64))
    assert V.d1[:, 0].tolist() == [16382, 0] and V.d2[0] == 268369924 == 16382 ** 2 and V.d2[1] == -268369924
    assert V.d2.max() == 268369924 and V.d2.min() == -268369924 and 2 * 268369924 < 2 ** 31


@pytest.mark.parametrize("Nk", [7, 45, 64, 130])
def test_lean_sk_slice_is_the_plain_one(pkg, oracle, Nk):
    """SliceSKLean against re_reference.SliceSK: same energy, same fields, and the same standardMC trajectory of an ensemble built on either"""
    import re_reference as RE
    X = pkg.GraphSKRE(Nk, 4, 1.0, 1.0, seed=Nk)
    J8 = LI.sk_bits(X.J, Nk)
    rng = np.random.default_rng(Nk)
    s = rng.integers(0, 2, Nk).astype(np.int64)
    plain, lean = RE.SliceSK(X.J, Nk), LI.SliceSKLean(J8, Nk)
    assert plain.energy(s) == lean.energy(s.copy()) and (plain.lf == lean.lf).all()
    a, b = RE.make_ensemble(Nk, 4, 1.0, 1.0, "sk", X.J), RE.make_ensemble(Nk, 4, 1.0, 1.0, "empty")
    b.X1 = [LI.SliceSKLean(J8, Nk) for _ in range(4)]
    sa = rng.integers(0, 2, 4 * Nk).astype(np.int64)
    sb = sa.copy()
    ra = RE.standard_mc(a, sa, 1.0, 600, 20, 5, oracle)
    rb = RE.standard_mc(b, sb, 1.0, 600, 20, 5, oracle)
    assert ra == rb and (sa == sb).all() and 0 < ra[2] < 600
    for k in range(4):
        assert (a.X1[k].lf == b.X1[k].lf).all()


def test_ens_build_is_declared_for_the_ensembles_only():
    src = open(os.path.join(ROOT, "rrrmc.jl_amd", "csrc", "rrrmc_hip.hip")).read()
    body = src[src.index("int32_t rrrmc_ens_build("):]
    body = body[:body.index("\n}\n")]
    assert "!is_re(ctx) && !is_le(ctx)" in body and "RRRMC_ERR_STATE" in body and "ctx->kids[0]" in body


@pytest.mark.parametrize("name", [n for n in LI.NAMES if "crafted_int16" in n])
def test_crafted_perceptron_energy_is_the_definition(pkg, oracle, name):
    e = LI.BY_NAME[name]
    sp = e.spec
    c, xi = LI.crafted_patterns(sp["N"], sp["crafted"], sp["seed"])
    n = LI.perc_energy_definition(xi.astype(np.int64), sp["linear"], c)
    ref = LI.reference(pkg, oracle, name)
    if sp["linear"]:
        assert n == 2048 * 16384 and ref[0]["E0"] == 2 * n / math.sqrt(32767) == 2 * 2048 * 16384 / math.sqrt(32767)
    else:
        assert n == 2040 and ref[0]["E0"] == 2040
    # and the stabilities walk away from the ends together: h net flips leave the two blocks at ±(32767 - 2 h)
    s = ref[0]["calls"][0]["s"]
    h = int((s != c).sum())
    d = LI.perc_deltas(xi.astype(np.int64), s)
    assert h > 0 and d.max() == 32767 - 2 * h and d.min() == -(32767 - 2 * h)


def test_gpu_test_runs_the_whole_table():
    import test_gpu_limits as G
    marks = [m for m in G.test_limit_instance.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and list(marks[0].args[1]) == LI.NAMES
    assert {m.name for m in G.test_limit_instance.pytestmark} == {"parametrize"}          # no skip, no xfail
    pm = G.pytestmark if isinstance(G.pytestmark, list) else [G.pytestmark]
    assert [m.name for m in pm] == ["gpu"]
