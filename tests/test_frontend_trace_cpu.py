"""The Python front end against its recorded call traces (tests/golden/frontend_traces.json, written by tests/golden/make_frontend_traces.py):
every C-ABI call ``Engine`` and the five sampler functions make — names, scalars, the crc32 of every array handed over — what each hook call
sees, what comes back and what is printed, for every graph family.  The library is replaced by the generator's recording stand-in, so no
device is needed: a change of engine.py / graphs.py that alters one call, one argument or their order fails here."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "frontend_traces.json")) as _f:
    EXPECTED = json.load(_f)


@pytest.fixture(scope="module")
def recorded():
    spec = importlib.util.spec_from_file_location("make_frontend_traces", os.path.join(GOLDEN, "make_frontend_traces.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    pkg, L, rec = gen.load()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(L, "_lib", rec)
        out = gen.generate(pkg, rec)
    return json.loads(json.dumps(out))          # tuples -> lists, as the golden file holds them


def test_same_cases(recorded):
    assert sorted(recorded) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_trace(recorded, case):
    got, want = recorded[case], EXPECTED[case]
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], "%s: %s differs" % (case, key)


def test_failed_upload_destroys_the_context():
    for case, want in EXPECTED.items():
        if case.startswith("upload-fails"):
            assert want["raised"] == 3 and want["graph_engine_unlinked"]
            assert want["calls"][-1] == "ctx_destroy(ctx)" and sum(c.startswith("set_") for c in want["calls"]) == 1


def test_raising_hook_leaves_resume_off():
    n = 0
    for case, want in EXPECTED.items():
        if "raise-at-2" in case:
            n += 1
            assert want["raised"] and len(want["hook"]) == 2
            tail = [c for c in want["calls"] if c.startswith(("set_resume", "ctx_destroy"))][-2:]
            assert tail == ["set_resume(ctx, 0)", "ctx_destroy(ctx)"]
    assert n == 11
