"""GraphQuant over pattern-machine slices (GraphQPercStepT ...): the Python restatement (tests/quant_pattern_reference.py) checks itself — tracked
energy against a fresh energy(X, C) after every iteration, cache consistency, the stream contract against the quant-RRG oracle — and checks
the preconditions of every GPU parity case; and the front ends' constructors are checked without a device."""
import os
import re

import numpy as np
import pytest

import quant_pattern_reference as QP
from re_reference import config_from_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _start(oracle, X, replica=0):
    return config_from_chunks(oracle.init_configs(QP.SEED, replica, 1, X.N)[0], X.N)


@pytest.mark.parametrize("case", QP.CASES, ids=QP.CASE_IDS)
def test_reference_tracks_the_energy_and_gpu_case_takes_every_branch(pkg, oracle, case):
    """RRRMC.jl:250 after every iteration; check_consistency; and what the GPU parity case relies on: the run takes the staged and the direct
    branch (0 < staged iterations < iters) and both accepts and rejects in each."""
    X = QP.make_graph(pkg, case)
    ref, fresh = QP.make_reference(X), QP.make_reference(X)
    s = _start(oracle, X)
    run = QP.RrrRun(ref, s, QP.BETA[case[1]], QP.SEED, oracle, staged_thr=QP.STAGED_THR, fresh_energy=lambda c: fresh.energy(np.array(c)))
    Es = run.run(QP.ITERS, QP.STEP)
    run.cache.check(s)
    assert len(Es) == QP.ITERS // QP.STEP
    assert [fresh.X1[k].energy(ref.C1[k]) for k in range(X.M)] == ref.renergies()
    for k in range(X.M):
        assert (ref.C1[k] == s[k * X.Nk:(k + 1) * X.Nk]).all()
    assert 0 < run.staged_its < QP.ITERS
    seen = set(run.branches)
    assert seen == {(True, True), (True, False), (False, True), (False, False)}, seen
    # standardMC on the same graph: the tracked energy is the fresh one at the end, and it both accepts and rejects
    s2 = _start(oracle, X)
    ref2 = QP.make_reference(X)
    Es2, E2, acc2 = QP.standard_mc(ref2, s2, QP.BETA[case[1]], QP.ITERS, QP.STEP, QP.SEED, oracle)
    assert abs(E2 - fresh.energy(s2)) < 1e-10 and 0 < acc2 < QP.ITERS


def test_trotter_part_reproduces_the_quant_rrg_oracle(oracle):
    """The stream contract: with slices of zero energy the chain is GraphQT's alone, and it is the oracle's rrrMC on a GraphQuant whose slice
    couplings are all zero — energies, classes, counts, final configuration and cache."""
    Nk, M, beta, Gamma, iters, step, seed = 16, 4, 1.3, 0.7, 800, 40, 0x51DE
    fourK = QP.quant_fourK(beta, Gamma, M)
    A = oracle.gen_rrg(Nk, 3, 5)
    J = np.zeros((Nk, 3), np.int32)
    ch0 = oracle.init_configs(seed, 0, 1, Nk * M)[0]
    Es_o, ch_o, acc_o, st_o, pos_o, sizes_o = oracle.rrr_mc_quant(A, J, M, fourK, beta, iters, step, seed, ch0, staged_thr=0.6, want_cache=True)
    s = config_from_chunks(ch0, Nk * M)
    X = QP.GraphQuantRef(Nk, M, fourK, [QP.SliceZero() for _ in range(M)])
    run = QP.RrrRun(X, s, beta, seed, oracle, staged_thr=0.6)
    Es = run.run(iters, step)
    run.cache.check(s)
    assert (np.array(Es) == Es_o).all()
    assert (s == config_from_chunks(ch_o, Nk * M)).all()
    assert (run.accepted, run.staged_its) == (acc_o, st_o) and 0 < st_o < iters
    pos, sizes = run.cache_view()
    assert (pos == pos_o).all() and (sizes == sizes_o).all()
    # standardMC likewise
    Es_s, ch_s, acc_s = oracle.standard_mc_quant(A, J, M, fourK, beta, iters, step, seed, ch0)
    s = config_from_chunks(ch0, Nk * M)
    Es2, _, acc2 = QP.standard_mc(QP.GraphQuantRef(Nk, M, fourK, [QP.SliceZero() for _ in range(M)]), s, beta, iters, step, seed, oracle)
    assert (np.array(Es2) == Es_s).all() and acc2 == acc_s and (s == config_from_chunks(ch_s, Nk * M)).all()


def test_constructors_mirror_the_reference(pkg):
    """src/QAliases.jl:85-159: both signatures, fourK rounded to 8 digits (QT.jl:165), the selectors of rrrmc_ctx_create_multi, the
    reference's argument errors"""
    X = pkg.GraphQPercStepT(33, 65, 3, 0.6, 2.0, seed=17)
    assert (X.N, X.Nk, X.M, X.pat_slices, X.model_kind) == (99, 33, 3, 3, 3) and X.fourK == QP.quant_fourK(2.0, 0.6, 3)
    assert (X.X1.xi == pkg.GraphPercStep(33, 65, seed=17).xi).all()
    assert X._multi_args() == (29, 33, 0, 3)
    Y = pkg.GraphQPercStepT(X.X1, 5, 0.3, 1.0)
    assert Y.X1 is X.X1 and Y.M == 5 and Y.fourK == QP.quant_fourK(1.0, 0.3, 5)
    assert pkg.GraphQPercLinearT(33, 65, 3, 0.6, 2.0)._multi_args() == (30, 33, 0, 3)
    C = pkg.GraphQCommStepT(3, 5, 9, 4, 0.6, 2.0, fc=True, seed=5)
    assert C._multi_args() == (31, 15, 5, 4) and (C.X1.xi == pkg.GraphCommStep(3, 5, 9, fc=True, seed=5).xi).all()
    Rl = pkg.GraphQCommReLUT(pkg.GraphCommReLU(4, 2, 9, seed=5), 3, 0.6, 2.0)
    assert Rl._multi_args() == (32, 8, 2, 3) and Rl.pat_slices == 6
    with pytest.raises(ValueError):
        pkg.GraphQPercStepT(32, 10, 3, 0.6, 2.0)                 # N even (PercStep.jl:57)
    with pytest.raises(ValueError):
        pkg.GraphQCommStepT(4, 3, 10, 3, 0.6, 2.0)               # K1 even (CommStep.jl:65)
    with pytest.raises(ValueError):
        pkg.GraphQCommReLUT(3, 2, 10, 3, 0.6, 2.0)               # K1 odd (CommReLU.jl:68)
    with pytest.raises(ValueError):
        pkg.GraphQPercStepT(33, 10, 2, 0.6, 2.0)                 # M > 2 (QT.jl:47)
    with pytest.raises(TypeError):
        pkg.GraphQPercLinearT(X.X1, 3, 0.6, 2.0)                 # a step graph for the linear alias
    with pytest.raises(TypeError):
        pkg.GraphQPercStepT(33, 65, 3, 0.6)                      # neither signature
    for name in ("GraphQPercStepT", "GraphQPercLinearT", "GraphQCommStepT", "GraphQCommReLUT", "Renergies", "Qenergy", "transverse_mag", "overlaps"):
        assert name in pkg.__all__


def test_julia_binding_reaches_the_pattern_quant_graphs():
    """The Julia file cannot be executed here: its text is checked.  A GraphQuant whose slice type is a pattern machine is created through
    rrrmc_ctx_create_quant_pattern (one device) or the four selectors 29 .. 32 (several), gets its patterns through the existing setters, and
    the reference's own Renergies has a method on OnGPU.  (tests/test_julia_binding.py checks every ccall's signature against the header.)"""
    src = open(os.path.join(ROOT, "julia", "RRRMCHip.jl")).read()
    m = re.search(r"elseif G <: Union\{PercGraph,CommGraph\}(.*?)elseif G <: F64Graph", src, re.S)
    assert m, "no pattern-machine branch in Ctx(X::GraphQuant, ...)"
    body = m.group(1)
    assert ":rrrmc_ctx_create_quant_pattern" in body and "QUANT_PAT_MODELS[kind - 2]" in body and "set_patterns!" in body
    assert re.search(r"const QUANT_PAT_MODELS = \(29, 30, 31, 32\)", src)
    assert ":rrrmc_quant_renergies" in src and "function RRRMC.QT.Renergies(G::OnGPU, " in src
    assert re.search(r"rrrmc_quant_set_field", src[m.end():]), "the field is set after the branch, as for every GraphQuant"
    hdr = open(os.path.join(ROOT, "include", "rrrmc_hip.h")).read()
    for k, name in enumerate(("PERC_STEP", "PERC_LINEAR", "COMM_STEP", "COMM_RELU")):
        assert re.search(r"RRRMC_MODEL_QUANT_%s = %d\b" % (name, 29 + k), hdr)
