"""GPU parity for GraphMixed (src/graphs/Mixed.jl) under standardMC: the thread build and the wavefront build, each forced and named by
``rrrmc_mixed_build``, equal the plain-Python restatement (tests/mixed_reference.py) bit for bit — sampled energies, accepted counts, final
spins, the tracked energy and the components' energies — on the instances of tests/mixed_instances.py, at the edges of β, in resumed and
two-shard runs, and with the debug checks on in every run.  No tolerances anywhere."""
import numpy as np
import pytest

import add_fields_reference as AF
import mixed_instances as MI
import mixed_reference as MR
import re_reference as RE

pytestmark = pytest.mark.gpu

ITERS, STEP = 1000, 7
BUILDS = [MI.THREAD, MI.WAVE]


@pytest.mark.parametrize("R", [1, 33])
@pytest.mark.parametrize("build", BUILDS, ids=["thread", "wave"])
@pytest.mark.parametrize("beta", [0.0, 0.7, 40.0])
@pytest.mark.parametrize("name", ["odd15", "even8", "n65", "xentr33", "int21"])
def test_standard_mc_bit_exact(pkg, oracle, name, beta, build, R):
    X = MI.mix(pkg, name)
    out = MI.run_standard(pkg, X, R, beta, [ITERS], STEP, build=build)
    assert out["Es"].shape == (R, ITERS // STEP)
    chains = MI.check_standard(oracle, X, out, R, beta, ITERS, STEP)
    # mixed_energies sums to energy, from the left, before and after the run
    for parts, tot in ((out["parts0"], out["E0"]), (out["parts1"], out["Etr"])):
        for r in range(R):
            E = parts[r][0]
            for e in parts[r][1:]:
                E = E + e
            assert abs(E - tot[r]) <= (0.0 if parts is out["parts0"] else 1e-10), (r, E, tot[r])
    if name == "int21":
        assert X.energy_dtype == np.int64 and (out["Es"] == np.round(out["Es"])).all()
    if beta == 0.0 and name in ("odd15", "even8"):
        # every move is accepted: consecutive flips of one site took GraphSKNormal's swap and the sparse graph's undo record
        m = chains[0]
        assert out["acc"][0] == ITERS and m.spf_undos >= 1 and (name == "even8" or m.skn_swaps >= 1)


@pytest.mark.parametrize("build", BUILDS, ids=["thread", "wave"])
@pytest.mark.parametrize("beta", [-1.0, float("inf")], ids=["negative", "inf"])
def test_the_edges_of_beta(pkg, oracle, beta, build):
    """β < 0 and β = +∞ run as the restatement does (at +∞ a move with ΔE = 0 has x = NaN and is rejected); NaN is refused"""
    X = MI.mix(pkg, "odd15")
    out = MI.run_standard(pkg, X, 33, beta, [ITERS], STEP, build=build)
    MI.check_standard(oracle, X, out, 33, beta, ITERS, STEP)
    with pkg.Engine(X, 1) as eng:
        eng.seed(1)
        eng.init_spins_random()
        with pytest.raises(pkg.RRRMCError) as e:
            eng.standard_mc(float("nan"), 10, 1)
        assert e.value.code == 1 and "NaN" in str(e.value)


@pytest.mark.parametrize("build", BUILDS, ids=["thread", "wave"])
@pytest.mark.parametrize("name", ["odd15", "n65"])
def test_resumed_calls_equal_the_run_in_one_call(pkg, oracle, name, build):
    """1000 iterations cut into 63, 1, 64, 65 and 807 (the wave build draws 64 iterations at a time): the chain is the chain of one call —
    final spins, accepted counts, tracked energy, components' energies.  A standardMC call samples every `step` iterations of the CALL (the
    library's standing rule for resumed standardMC calls, which the hooked-run loop cuts at sample points), so the samples of these pieces
    are held to the restatement run in the same pieces; cut at sample points (63, 7, 63, 70, 797) the samples are the one call's too."""
    X = MI.mix(pkg, name)
    pieces = [63, 1, 64, 65, 807]
    whole = MI.run_standard(pkg, X, 3, 0.7, [ITERS], STEP, build=build)
    cut = MI.run_standard(pkg, X, 3, 0.7, pieces, STEP, build=build)
    aligned = MI.run_standard(pkg, X, 3, 0.7, [63, 7, 63, 70, 797], STEP, build=build)
    for k in ("acc", "Etr", "parts1"):
        assert (whole[k] == cut[k]).all() and (whole[k] == aligned[k]).all(), k
    assert (whole["C1"].s == cut["C1"].s).all() and (whole["C1"].s == aligned["C1"].s).all()
    assert (whole["Es"] == aligned["Es"]).all()
    MI.check_standard(oracle, X, whole, 3, 0.7, ITERS, STEP, replicas={0, 2})
    for r in (0, 2):
        s = RE.config_from_chunks(cut["C0"].s[r], X.N)
        ref, E, it0, es = MR.as_chain(X), None, 0, []
        for n in pieces:
            e, E, _ = AF.standard_mc(ref, s, 0.7, n, STEP, MI.SEED, oracle, replica=r, it0=it0, E=E)
            es += [float(x) for x in e]
            it0 += n
        assert cut["Es"][r].tolist() == es and float(cut["Etr"][r]) == float(E), r


def test_the_order_of_the_list_is_part_of_the_model(pkg, oracle):
    """(SKN, SK, RRGNormal) and (RRGNormal, SK, SKN) each equal their restatement, and the two restatement runs differ"""
    beta = 0.7
    outs = {}
    for name in ("order-a", "order-b"):
        X = MI.mix(pkg, name)
        for build in BUILDS:
            out = MI.run_standard(pkg, X, 33, beta, [ITERS], STEP, build=build)
            MI.check_standard(oracle, X, out, 33, beta, ITERS, STEP)
            outs[name, build] = out
        assert (outs[name, MI.THREAD]["Es"] == outs[name, MI.WAVE]["Es"]).all()
    a, b = outs["order-a", MI.WAVE], outs["order-b", MI.WAVE]
    assert (a["C0"].s == b["C0"].s).all()
    assert (a["Es"] != b["Es"]).any(), "the two orders gave the same Float64 sums in every sample: the case shows nothing"


@pytest.mark.parametrize("build", BUILDS, ids=["thread", "wave"])
def test_two_shards_equal_one(pkg, build):
    X = MI.mix(pkg, "odd15")
    one = MI.run_standard(pkg, X, 33, 0.7, [ITERS], STEP, build=build)
    two = MI.run_standard(pkg, X, 33, 0.7, [ITERS], STEP, build=build, devices=[0, 0])
    for k in ("E0", "parts0", "Es", "acc", "Etr", "parts1"):
        assert (one[k] == two[k]).all(), k
    assert (one["C0"].s == two["C0"].s).all() and (one["C1"].s == two["C1"].s).all()


def test_the_default_build_and_a_hooked_run(pkg, oracle):
    """without a forced build 33 chains run the wave build; a hooked standardMC (resumed calls inside) is the chain of one call, and
    mixed_energies / step_energy read the live configuration inside the hook"""
    X = MI.mix(pkg, "xentr33")
    out = MI.run_standard(pkg, X, 33, 0.7, [ITERS], STEP)
    assert out["build"] == MI.WAVE
    seen = []

    def hook(it, Xh, C, acc, E):
        parts = np.atleast_2d(pkg.mixed_energies(Xh))
        seen.append((it, float(parts[0][0] + parts[0][1]), float(np.atleast_1d(E)[0]), int(np.atleast_1d(pkg.step_energy(Xh))[0])))
        return True
    Es, Cfg = pkg.standardMC(X, 0.7, 210, step=70, seed=MI.SEED, hook=hook, quiet=True)
    assert [x[0] for x in seen] == [70, 140, 210] and all(abs(x[1] - x[2]) < 1e-10 and 0 <= x[3] <= 5 for x in seen)
