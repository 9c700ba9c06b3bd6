"""What rrrmc_ctx_create_re / _le / _tle refuse, and in which words.  The creators check their arguments before they ask for a device, so every
refusal here is reached without a GPU; calls that pass the checks (their text depends on the machine) are left out.  Return code and
rrrmc_last_error(NULL) of every case are compared with tests/golden/ens_refusals.json, which was recorded by running this file's probe
(python tests/test_ens_refusals_cpu.py OUT.json, RRRMC_HIP_LIB naming the library) against a library built from the commit before the three
creators were folded into ens_ctx_create (host_ens.hpp): the error codes and texts of the ABI did not change with it."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ens_refusals.json")
M_MAX = {"re": 32, "le": 31, "tle": 31}          # kReMmax, kLeMmax, kTleMmax
OK_ARGS = dict(Nk=5, M=3, slice_kind=0, R=2, device=0, replica0=0)
EMPTY, SK, SKN, PERC_STEP, PERC_LINEAR, COMM_STEP, COMM_RELU, SAT, COMM_QU = 0, 1, 2, 3, 4, 5, 6, 8, 9


def cases():
    """(name, creator, out is NULL, arguments): one per refused argument class and creator."""
    out = []
    for fam in ("re", "le", "tle"):
        def add(name, null_out=False, **kw):
            out.append(("%s:%s" % (fam, name), fam, null_out, dict(OK_ARGS, **kw)))
        big = M_MAX[fam] + 1
        add("out_null", null_out=True)
        for s in (-1, 7, 10):
            add("slice_%d" % s, slice_kind=s)
        if fam == "tle":
            for s in (PERC_STEP, PERC_LINEAR, COMM_STEP, COMM_RELU, COMM_QU):
                add("slice_unsupported_%d" % s, slice_kind=s)
            add("slice_unsupported_and_m_2", slice_kind=PERC_STEP, M=2)
        else:
            for s in (PERC_STEP, PERC_LINEAR):
                add("perc_%d_even_nk" % s, slice_kind=s, Nk=4)
                add("perc_%d_nk_too_large" % s, slice_kind=s, Nk=32769)
            add("comm_step_even_nk", slice_kind=COMM_STEP, Nk=4)
            add("comm_step_nk_too_large", slice_kind=COMM_STEP, Nk=32769)
            for s in (COMM_RELU, COMM_QU):
                add("comm_%d_odd_nk" % s, slice_kind=s, Nk=5)
                add("comm_%d_nk_not_multiple_of_4" % s, slice_kind=s, Nk=6)
                add("comm_%d_nk_too_large" % s, slice_kind=s, Nk=32768)
            add("perc_even_nk_and_m_2", slice_kind=PERC_STEP, Nk=4, M=2)
        add("nk_0", Nk=0)
        add("nk_negative", Nk=-3)
        add("r_0", R=0)
        add("m_2", M=2)
        add("m_0", M=0)
        add("m_too_large", M=big)
        n_rows = 4 if fam == "re" else 3          # Nk*M (RE) or Nk*(M+1) (LE, TLE) = 65536 with Nk = 16384
        add("n_65536", Nk=16384, M=n_rows)
        add("n_above", Nk=20000, M=4)
        add("replica0_16", replica0=16)
        add("replica0_33", replica0=33)
        # two things wrong: the order of the checks decides the message
        add("bad_slice_and_m_2", slice_kind=7, M=2)
        add("nk_0_and_m_2", Nk=0, M=2)
        add("m_too_large_and_n_too_large", M=big, Nk=65536)
        add("bad_replica0_and_m_2", replica0=16, M=2)
    return out


def probe(lib):
    res = {}
    for name, fam, null_out, a in cases():
        ctx = C.c_void_p()
        fn = getattr(lib, "rrrmc_ctx_create_" + fam)
        rc = fn(None if null_out else C.byref(ctx), a["Nk"], a["M"], a["slice_kind"], a["R"], a["device"], a["replica0"])
        msg = lib.rrrmc_last_error(None)
        assert ctx.value is None, name
        res[name] = [int(rc), msg.decode() if msg else ""]
    return res


@pytest.fixture(scope="module")
def refusals(pkg):
    return probe(pkg.lib())


def test_every_refusal_is_the_recorded_one(refusals):
    with open(GOLDEN, encoding="utf-8") as fh:
        want = json.load(fh)
    assert sorted(refusals) == sorted(want)
    for name in sorted(want):
        assert refusals[name] == want[name], name


def test_the_recorded_refusals_are_refusals_before_any_device_query(refusals):
    names = [c[0] for c in cases()]
    assert len(names) == len(set(names)) == len(refusals)
    for name, (rc, msg) in refusals.items():
        assert rc in (1, 3) and msg, name                          # RRRMC_ERR_INVALID_ARG or RRRMC_ERR_UNSUPPORTED, with a text
        assert "HIP" not in msg and "device" not in msg, name      # (not the device query's)


if __name__ == "__main__":          # records the golden file: see the docstring
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as g
    with open(sys.argv[1], "w", encoding="utf-8") as fh:
        json.dump(probe(g.load_package().lib()), fh, indent=1, ensure_ascii=False, sort_keys=True)
        fh.write("\n")
