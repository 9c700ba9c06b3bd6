"""The rows of the ensemble-model table (rrrmc.jl_amd/csrc/ens_models.hpp) for the sparse Float64 slices: model ids 67, 68, 69 are the Robust
Ensemble, the Local Entropy ensemble and the Topological Local Entropy ensemble over slice kind 12, in both directions; slice kinds 11 and 13
name no ensemble model, and no other id of 48 .. 101 has a family.  The HIP-free header is compiled into a stand-alone program with
g++ -fsanitize=address,undefined (tests/sparse_ens_models_check.cpp), as tests/test_ens_models_cpu.py does for ids 0 .. 47."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, RE, LE, TLE = 0, 1, 2, 3
NO_MODEL, NO_SLICE, SPARSE_F64 = 0, -1, 12
MODELS = {67: (RE, SPARSE_F64), 68: (LE, SPARSE_F64), 69: (TLE, SPARSE_F64)}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("sparse_ens_models") / "sparse_ens_models_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "sparse_ens_models_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    by_model, by_pair = {}, {}
    for f in (l.split() for l in out.stdout.splitlines()):
        if f[0] == "M":
            by_model[int(f[1])] = (int(f[2]), int(f[3]))
        else:
            assert f[0] == "P"
            by_pair[(int(f[1]), int(f[2]))] = int(f[3])
    assert sorted(by_model) == list(range(48, 102))
    assert sorted(by_pair) == [(fam, s) for fam in range(4) for s in (11, 12, 13)]
    return by_model, by_pair


def test_ids_67_to_69_are_the_three_ensembles_over_slice_kind_12(table):
    by_model, by_pair = table
    for model, (fam, s) in MODELS.items():
        assert by_model[model] == (fam, s)
        assert by_pair[(fam, s)] == model


def test_no_other_id_of_48_to_101_has_a_family(table):
    by_model, _ = table
    for model in range(48, 102):
        if model not in MODELS:
            assert by_model[model] == (NONE, NO_SLICE), model
    for model in range(48, 67):          # the field wrappers and GraphPercXEntr
        assert by_model[model] == (NONE, NO_SLICE), model


def test_kinds_11_and_13_and_the_family_none_name_no_model(table):
    _, by_pair = table
    for fam in (NONE, RE, LE, TLE):
        assert by_pair[(fam, 11)] == NO_MODEL          # GraphPercXEntr: the g of the field wrappers only
        assert by_pair[(fam, 13)] == NO_MODEL
    assert by_pair[(NONE, SPARSE_F64)] == NO_MODEL
