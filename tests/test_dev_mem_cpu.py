"""The registry of a context's device allocations (rrrmc.jl_amd/csrc/dev_mem.hpp).  The HIP-free header is compiled with g++ into a stand-alone
program (tests/dev_mem_check.cpp) with the sanitizers on, as tests/test_ens_models_cpu.py does with the ensembles' table: its raw hooks count
the live blocks over malloc / free, and the sanitizer's leak and double-free reports are part of the pass.  The source-text tests below are
the structural half: nothing under csrc/ allocates or frees device memory past the registry, and rrrmc_ctx_destroy names no buffer."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rrrmc.jl_amd", "csrc")
SCENARIOS = ["alloc_then_free", "failing_alloc", "grow", "grow_that_fails", "pointers_in_a_vector_that_moves", "free_all_after_a_mix",
             "free_of_null_and_of_a_stranger", "all"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("dev_mem") / "dev_mem_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "dev_mem_check.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_the_program_ends_clean_under_the_sanitizers(run):
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == ""          # no leak, no double free, no undefined behaviour reported


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(run, name):
    assert "ok %s" % name in run.stdout.splitlines(), run.stdout + run.stderr


def _sources():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, encoding="utf-8") as fh:
            yield os.path.basename(path), fh.read().splitlines()


def test_device_memory_is_allocated_and_freed_through_the_registry_only():
    """hipMalloc( and hipFree( occur in dev_mem.hpp's two raw hooks (defined in rrrmc_hip.hip) and in two allocations no context owns: the
    local buffers of rrrmc_device_copy_bandwidth and g_stamps under RRRMC_STAMPS."""
    allowed = {
        "hipError_t dev_raw_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }": 1,
        "void dev_raw_free(void* p) { (void)hipFree(p); }": 1,
        "if (e == hipSuccess) e = hipMalloc(&a, (size_t)nbytes);": 1,
        "if (e == hipSuccess) e = hipMalloc(&b, (size_t)nbytes);": 1,
        "if (a) (void)hipFree(a);": 1,
        "if (b) (void)hipFree(b);": 1,
        "if (!g_stamps) HIP_TRY(ctx, hipMalloc(&g_stamps, sizeof(unsigned long long) * 16 * (65536 + 4096)));": 2,
    }
    seen = {}
    for name, lines in _sources():
        for n, line in enumerate(lines, 1):
            assert "free_dev" not in line, "%s:%d" % (name, n)
            if "hipMalloc(" in line or "hipFree(" in line:
                code = line.strip()
                assert code in allowed and name in ("rrrmc_hip.hip", "host_sweep.hpp"), "%s:%d: %s" % (name, n, code)
                seen[code] = seen.get(code, 0) + 1
    assert seen == allowed


def test_one_creation_macro():
    """no _TRY macro other than HIP_TRY and CTX_CREATE_TRY under csrc/"""
    names = set()
    for _, lines in _sources():
        names.update(re.findall(r"\b\w+_TRY\b", "\n".join(lines)))
    assert names == {"HIP_TRY", "CTX_CREATE_TRY"}


def test_destroy_names_no_buffer():
    lines = dict(_sources())["rrrmc_hip.hip"]
    text = "\n".join(lines)
    struct = text[text.index("struct rrrmc_ctx {"):text.index("\n};", text.index("struct rrrmc_ctx {"))]
    fields = set(re.findall(r"\*\s*(\w+)\s*(?:\[\d+\])?\s*=\s*\{?\s*nullptr", struct)) | {"d_color_list"}          # every pointer member, and the vector of colour lists
    assert {"d_A", "d_slots", "d_pairs", "sk_Es", "dbg_lfl", "pff_thr_lo"} <= fields and len(fields) > 120
    not_device = {"stream", "plan_stream", "ev_upload", "ev_begin", "ev_end", "ev_set_free", "h_chunks"}          # streams, events, pinned host memory
    start = text.index("void rrrmc_ctx_destroy(rrrmc_ctx* ctx)\n{")
    body = text[start:text.index("\n}\n", start)]
    assert "dev_free_all(ctx);" in body
    used = set(re.findall(r"ctx->(\w+)", body))
    assert used & not_device == {"stream", "plan_stream", "ev_upload", "ev_begin", "ev_end", "ev_set_free", "h_chunks"}
    assert used & (fields - not_device) == set()
