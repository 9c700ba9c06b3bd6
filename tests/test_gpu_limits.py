"""GPU parity at the size limits (tests/limit_instances.py): every entry of the table — the perceptrons at N = 32767 and P = 4096 and with
stabilities on both ends of an int16, the ensembles and the field wrappers at N = 65535 and M on its bound, and the pairs of adjacent shapes
on both sides of the LDS-fit rule — runs two consecutive sampler calls with the debug checks on and equals the plain-Python reference bit
for bit: start configuration, energy(X, C), sampled energies, accepted and staged counts, final configuration, tracked energy, the
sampler's cache and the ensembles' observables.  Where the family has a build reporter, the build it names is asserted: for a boundary
pair, LDS on the first shape and global memory on the second, with no switch set.  The pairs of the cross-entropy table and of the sparse
slices' state have no reporter of their own (rrrmc_xentr_build and rrrmc_ens_build name the same build on both sides): parity pins them."""
import os

import numpy as np
import pytest

import limit_instances as LI

pytestmark = pytest.mark.gpu

SWITCHES = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS", "RRRMC_LE_NO_LDS", "RRRMC_LE_LDS", "RRRMC_AF_NO_LDS", "RRRMC_XENTR_WAVE", "RRRMC_XENTR_NO_WAVE",
            "RRRMC_XENTR_NO_LDS", "RRRMC_SAT_NO_WAVE", "RRRMC_QUANT_NO_WAVE", "RRRMC_QUANT_NO_LDS", "RRRMC_QUANT_WAVE_MAX_R")


class _env:
    """The library reads every build switch with getenv when a sampler call is launched (host_re.hpp:116, host_le.hpp:148, host_af.hpp:199,
    host_sat.hpp:129, host_xentr.hpp:74, host_quant_pat.hpp:50), not when the context is made — which is why the reporters name the build of
    the last call.  The block holds the environment from before the context is created until after its last call, so it is right under
    either reading: none of the switches is set unless the entry names it."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k in SWITCHES:
            os.environ.pop(k, None)
            if self.old[k] is not None:
                os.environ[k] = self.old[k]


def _reporter(eng, family):
    return {"re": eng.ens_build, "le": eng.ens_build, "af": eng.af_build, "xentr": eng.xentr_build, "sat": eng.sat_build, "quant": eng.quant_pattern_build}.get(family)


@pytest.mark.parametrize("name", LI.NAMES)
def test_limit_instance(pkg, oracle, name):
    e = LI.BY_NAME[name]
    rn = e.run
    R, iters, step, beta = rn["R"], rn["iters"], rn["step"], rn["beta"]
    X = LI.graph(pkg, name)
    N = X.N
    ref = LI.reference(pkg, oracle, name)
    C0 = LI.start_configs(pkg, oracle, name)
    rrr = rn["sampler"] != "std"
    with _env(e.env), pkg.Engine(X, R) as eng:
        eng.set_debug_checks(True)
        eng.seed(rn["seed"])
        if e.spec.get("start"):
            eng.set_config(pkg.graphs.Config(N, R, C0.copy()))
        else:
            eng.init_spins_random()
        assert (eng.get_config().s == C0).all()
        E0 = np.atleast_1d(eng.energy())
        assert E0.dtype == X.energy_dtype
        build = _reporter(eng, e.family)
        if build is not None and e.family != "quant":          # (rrrmc_quant_pattern_build answers for the next call too: no "none yet")
            assert build() == 0
        calls = []
        for c in range(2):                      # the second call continues the streams (not the run: resume is off)
            if rrr:
                Es, acc, staged = eng.rrr_mc(beta, iters, step, staged_thr=rn["thr"])
                cache = eng.af_cache() if e.family == "af" else eng.rrr_cache()
            else:
                (Es, acc), staged, cache = eng.standard_mc(beta, iters, step), None, None
            if e.family == "xentr":
                assert np.atleast_1d(eng.step_energy()).tolist() == [ref[r]["step_energy"][c] for r in range(R)]
            calls.append((np.atleast_2d(Es).copy(), np.atleast_1d(acc).copy(), None if staged is None else np.atleast_1d(staged).copy(),
                          eng.get_config().s.copy(), np.atleast_1d(eng.run_energy()).copy(), cache))
            if e.build is not None:
                assert build() == e.build, (name, build(), e.lds)
        if e.family == "quant":
            obs = dict(renergies=np.atleast_2d(eng.quant_renergies()))
        elif e.family == "re":
            obs = dict(re=np.atleast_2d(eng.re_energies()))
        elif e.family == "le":
            obs = dict(le=np.atleast_2d(eng.le_energies()), c=np.atleast_1d(eng.cenergy()), d=np.asarray(eng.distances()).reshape(R, e.spec["M"], e.spec["M"]))
    for r in range(R):
        assert E0[r] == ref[r]["E0"], r
        for c in range(2):
            Es, acc, staged, C1, Etr, cache = calls[c]
            want = ref[r]["calls"][c]
            assert Es.shape == (R, iters // step)
            assert Es[r].tolist() == want["Es"], (r, c)
            assert acc[r] == want["acc"], (r, c)
            assert (C1[r] == LI.pack(want["s"])[0]).all(), (r, c)
            assert Etr[r] == want["E"], (r, c)
            if rrr:
                assert staged[r] == want["staged"], (r, c)
                if e.family == "af":
                    dEs, v, z, tref = want["cache"]
                    assert cache[0][r].tolist() == dEs and cache[1][r].tolist() == v and cache[2][r] == z and cache[3][r] == tref, (r, c)
                else:
                    pos, sizes = want["cache"]
                    assert (cache[0][r] == pos).all() and (cache[1][r] == sizes).all(), (r, c)
        if e.family == "quant":
            assert obs["renergies"][r].tolist() == ref[r]["obs"]["renergies"], r
        elif e.family == "re":
            assert obs["re"][r].tolist() == ref[r]["obs"]["re"], r
        elif e.family == "le":
            assert obs["le"][r].tolist() == ref[r]["obs"]["le"] and float(obs["c"][r]) == ref[r]["obs"]["c"], r
            assert obs["d"][r].tolist() == ref[r]["obs"]["d"], r


def test_ens_build_states_and_refusal(pkg):
    """0 before any call and after a standardMC-only run (standardMC has one build); RRRMC_ERR_STATE on a context that is no ensemble"""
    with pkg.Engine(pkg.Graph0RE(11, 3, 1.0, 1.0), 2) as eng:
        eng.seed(1)
        eng.init_spins_random()
        assert eng.ens_build() == 0
        eng.standard_mc(1.0, 100, 10)
        assert eng.ens_build() == 0
        eng.rrr_mc(1.0, 100, 10)
        assert eng.ens_build() == LI.LDS
        eng.standard_mc(1.0, 100, 10)
        assert eng.ens_build() == LI.LDS          # the build of the last rrrMC call
    with pkg.Engine(pkg.Graph0LE(11, 3, 1.0, 1.0), 2, devices=[0, 0]) as eng:          # two shards: the first one's answer
        eng.seed(1)
        eng.init_spins_random()
        assert eng.ens_build() == 0
        eng.rrr_mc(1.0, 100, 10)
        assert eng.ens_build() == LI.LDS
    with pkg.Engine(pkg.GraphPercStep(11, 5), 2) as eng:
        with pytest.raises(pkg.RRRMCError) as err:
            eng.ens_build()
        assert err.value.code == 2
