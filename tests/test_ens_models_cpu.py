"""The table of ensemble models (rrrmc.jl_amd/csrc/ens_models.hpp: model id <-> (ensemble, slice kind)) against the 22 rows of
include/rrrmc_hip.h spelled out here.  The HIP-free header is compiled with g++ into a stand-alone program (tests/ens_models_check.cpp)
with the sanitizers on, as tests/test_zero_blocks_cpu.py does with the planner's host code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, RE, LE, TLE = 0, 1, 2, 3
EMPTY, SK, SKN, PERC_STEP, PERC_LINEAR, COMM_STEP, COMM_RELU, SAT, COMM_QU = 0, 1, 2, 3, 4, 5, 6, 8, 9      # enum rrrmc_re_slice; 7 is unassigned
NO_MODEL, NO_SLICE = 0, -1
# enum rrrmc_model, the comments of its ensemble entries: model id -> (ensemble, slice kind)
MODELS = {
    11: (RE, EMPTY),            # Graph0RE
    12: (RE, SK),               # GraphSKRE
    13: (RE, SKN),              # GraphRobustEnsemble(..., GraphSKNormal, J)
    14: (LE, EMPTY),            # Graph0LE
    15: (LE, SK),               # GraphSKLE
    16: (LE, SKN),              # GraphLocalEntropy(..., GraphSKNormal, J)
    19: (RE, PERC_STEP),        # GraphPercStepRE
    20: (RE, PERC_LINEAR),      # GraphPercLinearRE
    21: (LE, PERC_STEP),        # GraphPercStepLE
    22: (LE, PERC_LINEAR),      # GraphPercLinearLE
    25: (RE, COMM_STEP),        # GraphCommStepRE
    26: (RE, COMM_RELU),        # GraphCommReLURE
    27: (LE, COMM_STEP),        # GraphCommStepLE
    28: (LE, COMM_RELU),        # GraphCommReLULE
    34: (RE, SAT),              # GraphSATRE
    35: (LE, SAT),              # GraphSATLE
    37: (RE, COMM_QU),          # GraphCommQuRE
    38: (LE, COMM_QU),          # GraphCommQuLE
    44: (TLE, EMPTY),           # Graph0TLE
    45: (TLE, SK),              # GraphSKTLE
    46: (TLE, SKN),             # GraphTopologicalLocalEntropy(..., GraphSKNormal, J)
    47: (TLE, SAT),             # GraphSATTLE
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("ens_models") / "ens_models_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "ens_models_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    by_model, by_pair = {}, {}
    for f in (l.split() for l in out.stdout.splitlines()):
        if f[0] == "M":
            by_model[int(f[1])] = (int(f[2]), int(f[3]))
        else:
            assert f[0] == "P"
            by_pair[(int(f[1]), int(f[2]))] = int(f[3])
    assert sorted(by_model) == list(range(48))
    assert sorted(by_pair) == [(fam, s) for fam in range(4) for s in range(-1, 11)]
    return by_model, by_pair


def test_the_22_ensemble_models_and_no_other(table):
    by_model, _ = table
    assert len(MODELS) == 22
    for model in range(48):
        assert by_model[model] == MODELS.get(model, (NONE, NO_SLICE)), model


def test_the_two_directions_are_inverse(table):
    by_model, by_pair = table
    for model, (fam, s) in MODELS.items():
        assert by_pair[(fam, s)] == model
    for (fam, s), model in by_pair.items():
        if model != NO_MODEL:
            assert by_model[model] == (fam, s)
    assert sorted(m for m in by_pair.values() if m != NO_MODEL) == sorted(MODELS)


def test_pairs_that_name_no_model(table):
    _, by_pair = table
    for fam in (NONE, RE, LE, TLE):
        for s in (-1, 7, 10):
            assert by_pair[(fam, s)] == NO_MODEL, (fam, s)
    for s in range(-1, 11):
        assert by_pair[(NONE, s)] == NO_MODEL
    for fam in (RE, LE):
        assert [s for s in range(-1, 11) if by_pair[(fam, s)] != NO_MODEL] == [EMPTY, SK, SKN, PERC_STEP, PERC_LINEAR, COMM_STEP, COMM_RELU, SAT, COMM_QU]
    # the Topological Local Entropy kernels cover GraphEmpty, GraphSK, GraphSKNormal and GraphSAT slices
    assert [s for s in range(-1, 11) if by_pair[(TLE, s)] != NO_MODEL] == [EMPTY, SK, SKN, SAT]
