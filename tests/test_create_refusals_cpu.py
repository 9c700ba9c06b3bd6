"""What the context creators refuse, and in which words: rrrmc_ctx_create (its six model kinds), the GraphQuant creators, the perceptron, the
committee machines, K-SAT and rrrmc_ctx_create_multi; tests/test_ens_refusals_cpu.py covers _re / _le / _tle.  Every creator checks its
arguments before it asks for a device, so every refusal here is reached without a GPU; calls that pass the checks (their text depends on the
machine) are left out.  Return code and rrrmc_last_error(NULL) of every case are compared with tests/golden/create_refusals.json, which was
recorded by running this file's probe (python tests/test_create_refusals_cpu.py OUT.json, RRRMC_HIP_LIB naming the library) against a library
built from the commit before the creators' shared frame (ctx_create_begin, CTX_CREATE_TRY in rrrmc_hip.hip) replaced their nine private copies:
the order of the checks, the error codes and the texts of the ABI did not change with it."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_refusals.json")
I32, I64, U32 = C.c_int32, C.c_int64, C.c_uint32
PM1, SKN, QUANT_RRG, SKB, F64, DISC, LEV = 1, 2, 3, 4, 5, 6, 7          # RRRMC_MODEL_*
PERC_STEP_M, COMM_STEP_M, COMM_RELU_M, SAT_M = 17, 23, 24, 33
S_PERC_STEP, S_PERC_LINEAR, S_COMM_STEP, S_COMM_RELU, S_COMM_QU = 3, 4, 5, 6, 9          # RRRMC_RE_SLICE_*

# creator -> (argument names after `out`, their C types, a set of arguments that passes every check)
SIGS = {
    "create": (("model", "N", "K", "R", "device", "replica0"), (I32, I64, I64, I64, I32, U32), dict(model=PM1, N=64, K=3, R=32, device=0, replica0=0)),
    "create_quant": (("Nk", "K", "M", "R", "device", "replica0"), (I64, I64, I64, I64, I32, U32), dict(Nk=16, K=3, M=4, R=4, device=0, replica0=0)),
    "create_quant_sk": (("Nk", "M", "R", "device", "replica0"), (I64, I64, I64, I32, U32), dict(Nk=16, M=4, R=4, device=0, replica0=0)),
    "create_quant_skn": (("Nk", "M", "R", "device", "replica0"), (I64, I64, I64, I32, U32), dict(Nk=16, M=4, R=4, device=0, replica0=0)),
    "create_quant_f64": (("Nk", "K", "M", "R", "device", "replica0"), (I64, I64, I64, I64, I32, U32), dict(Nk=16, K=3, M=4, R=4, device=0, replica0=0)),
    "create_quant_pattern": (("slice_kind", "Nk", "K2", "M", "R", "device", "replica0"), (I32, I64, I64, I64, I64, I32, U32),
                             dict(slice_kind=S_PERC_STEP, Nk=21, K2=0, M=4, R=4, device=0, replica0=0)),
    "create_perc": (("N", "linear", "R", "device", "replica0"), (I64, I32, I64, I32, U32), dict(N=21, linear=0, R=4, device=0, replica0=0)),
    "create_comm": (("K1", "K2", "relu", "R", "device", "replica0"), (I64, I64, I32, I64, I32, U32), dict(K1=3, K2=7, relu=0, R=4, device=0, replica0=0)),
    "create_comm_qu": (("K1", "K2", "R", "device", "replica0"), (I64, I64, I64, I32, U32), dict(K1=4, K2=6, R=4, device=0, replica0=0)),
    "create_sat": (("N", "R", "device", "replica0"), (I64, I64, I32, U32), dict(N=32, R=4, device=0, replica0=0)),
    # device_ids: a tuple of ids, or None for NULL
    "create_multi": (("model", "N", "K", "M", "R", "device_ids", "ndev", "replica0"), (I32, I64, I64, I64, I64, None, I32, U32),
                     dict(model=PM1, N=64, K=3, M=0, R=64, device_ids=(0,), ndev=1, replica0=0)),
}


def cases():
    """(name, creator, out is NULL, arguments): one per refused argument class and creator."""
    out = []

    def adder(fn, tag=None, **base):
        def add(name, null_out=False, **kw):
            out.append(("%s:%s" % (tag or fn, name), fn, null_out, dict(SIGS[fn][2], **dict(base, **kw))))
        return add

    def sizes(add, names):
        for a in names:
            add("%s_0" % a.lower(), **{a: 0})
            add("%s_negative" % a.lower(), **{a: -3})

    # ---- rrrmc_ctx_create ----
    add = adder("create")
    add("out_null", null_out=True)
    add("quant_rrg_redirect", model=QUANT_RRG)
    for m in (0, -1, 8, 17, 99):
        add("unknown_kind_%d" % m, model=m)
    add("out_null_and_unknown_kind", null_out=True, model=99)
    add("unknown_kind_and_n_0", model=99, N=0)
    add("quant_rrg_and_n_0", model=QUANT_RRG, N=0)
    for tag, model, kmax1, nmax1, r0 in (("pm1", PM1, 8, (2**31 - 1) // 8 + 1, True), ("f64", F64, 9, (2**31 - 1) // 64 + 1, False),
                                         ("disc", DISC, 9, 2**28 + 1, False), ("lev", LEV, 17, 2**28 + 1, False)):
        add = adder("create", "create_" + tag, model=model)
        sizes(add, ("N", "K", "R"))
        add("k_above", K=kmax1)
        add("n_above", N=nmax1)
        if r0:          # (the other three take any replica0: such a call reaches the device query)
            add("replica0_16", replica0=16)
            add("replica0_33", replica0=33)
            add("n_above_and_bad_replica0", N=nmax1, replica0=16)
        add("n_0_and_k_above", N=0, K=kmax1)
        add("k_above_and_n_above", K=kmax1, N=nmax1)
    for tag, model in (("skn", SKN), ("skb", SKB)):
        add = adder("create", "create_" + tag, model=model, N=32, K=0, R=8)
        sizes(add, ("N", "R"))
        add("n_4097", N=4097)
        add("replica0_16", replica0=16)
        add("replica0_33", replica0=33)
        add("n_0_and_bad_replica0", N=0, replica0=16)
        add("n_4097_and_bad_replica0", N=4097, replica0=16)
    # ---- GraphQuant ----
    for fn, has_k in (("create_quant", True), ("create_quant_sk", False), ("create_quant_skn", False), ("create_quant_f64", True)):
        add = adder(fn)
        add("out_null", null_out=True)
        sizes(add, ("Nk", "K", "R") if has_k else ("Nk", "R"))
        for M in (2, 0, -1):
            add("m_%d" % M, M=M)
        add("n_above", Nk=2**27, M=3)
        if fn == "create_quant_f64":
            add("k_9", K=9)
            add("m_2_and_k_9", M=2, K=9)
            add("k_9_and_n_above", K=9, Nk=2**27, M=3)
        add("nk_0_and_m_2", Nk=0, M=2)
        add("m_2_and_n_above", Nk=2**28, M=2)
        add("out_null_and_nk_0", null_out=True, Nk=0)
    add = adder("create_quant_pattern")
    add("out_null", null_out=True)
    for s in (-1, 0, 1, 2, 7, 8, 10):
        add("slice_%d" % s, slice_kind=s)
    for s in (S_PERC_STEP, S_PERC_LINEAR):
        add("perc_%d_even_nk" % s, slice_kind=s, Nk=20)
        add("perc_%d_nk_too_large" % s, slice_kind=s, Nk=32769)
    for s, k1, k2, big in ((S_COMM_STEP, 3, 7, 183), (S_COMM_RELU, 4, 6, 182), (S_COMM_QU, 4, 6, 182)):
        add("comm_%d_k2_0" % s, slice_kind=s, Nk=k1 * k2, K2=0)
        add("comm_%d_k2_negative" % s, slice_kind=s, Nk=k1 * k2, K2=-3)
        add("comm_%d_nk_not_multiple_of_k2" % s, slice_kind=s, Nk=k1 * k2 + 1, K2=k2)
        add("comm_%d_k1_parity" % s, slice_kind=s, Nk=(k1 + 1) * k2, K2=k2)
        add("comm_%d_k2_parity" % s, slice_kind=s, Nk=k1 * (k2 + 1), K2=k2 + 1)
        add("comm_%d_both_parities" % s, slice_kind=s, Nk=(k1 + 1) * (k2 + 1), K2=k2 + 1)
        add("comm_%d_n_too_large" % s, slice_kind=s, Nk=big * (big - 2 * (big % 2)), K2=big)
        add("comm_%d_k1_parity_and_m_2" % s, slice_kind=s, Nk=(k1 + 1) * k2, K2=k2, M=2)
    sizes(add, ("Nk", "R"))
    for M in (2, 0, -1):
        add("m_%d" % M, M=M)
    add("n_above", Nk=21845, M=4)
    add("bad_slice_and_nk_0", slice_kind=7, Nk=0)
    add("nk_0_and_m_2", Nk=0, M=2)
    add("even_nk_and_m_2", Nk=20, M=2)
    add("m_2_and_n_above", Nk=32767, M=2)
    # ---- perceptron, committee machines, K-SAT ----
    for linear in (0, 1):
        add = adder("create_perc", "create_perc_%d" % linear, linear=linear)
        add("out_null", null_out=True)
        sizes(add, ("N", "R"))
        add("n_even", N=20)
        add("n_32769", N=32769)
        add("replica0_16", replica0=16)
        add("replica0_33", replica0=33)
        add("n_0_and_bad_replica0", N=0, replica0=16)
        add("n_even_and_bad_replica0", N=20, replica0=16)
        add("n_even_and_too_large", N=32768)
    for fn, tag, base, k1, k2, big in (("create_comm", "create_comm_step", dict(relu=0), 3, 7, 183), ("create_comm", "create_comm_relu", dict(relu=1, K1=4, K2=6), 4, 6, 182),
                                       ("create_comm_qu", None, {}, 4, 6, 182)):
        add = adder(fn, tag, **base)
        add("out_null", null_out=True)
        sizes(add, ("R", "K1", "K2"))
        add("k1_parity", K1=k1 + 1)
        add("k2_parity", K2=k2 + 1)
        add("both_parities", K1=k1 + 1, K2=k2 + 1)
        add("n_too_large", K1=big, K2=big - 2 * (big % 2))
        add("replica0_16", replica0=16)
        add("replica0_33", replica0=33)
        add("r_0_and_k1_0", R=0, K1=0)
        add("k1_parity_and_bad_replica0", K1=k1 + 1, replica0=16)
        add("n_too_large_and_bad_replica0", K1=big, K2=big - 2 * (big % 2), replica0=16)
    add = adder("create_sat")
    add("out_null", null_out=True)
    sizes(add, ("N", "R"))
    add("n_65536", N=65536)
    add("replica0_16", replica0=16)
    add("replica0_33", replica0=33)
    add("n_0_and_bad_replica0", N=0, replica0=16)
    add("n_65536_and_bad_replica0", N=65536, replica0=16)
    # ---- rrrmc_ctx_create_multi: its own checks, then what the creator of the first shard refuses ----
    add = adder("create_multi")
    add("out_null", null_out=True)
    add("device_ids_null", device_ids=None)
    for n in (0, -1, 65):
        add("ndev_%d" % n, ndev=n, device_ids=(0,) * 65)
    sizes(add, ("R",))
    add("replica0_16", replica0=16)
    add("comm_k_0", model=COMM_STEP_M, N=21, K=0)
    add("comm_n_not_multiple_of_k", model=COMM_RELU_M, N=25, K=6)
    add("ndev_0_and_r_0", ndev=0, R=0)
    add("ndev_65_and_r_0", ndev=65, device_ids=(0,) * 65, R=0)
    add("r_0_and_bad_replica0", R=0, replica0=16)
    add("bad_replica0_and_comm_k_0", replica0=16, model=COMM_STEP_M, N=21, K=0)
    add("child_unknown_kind", model=99)
    add("child_pm1_k_8", K=8)
    add("child_pm1_n_0", N=0, device_ids=(0, 0), ndev=2)
    add("child_quant_m_2", model=QUANT_RRG, N=16, M=2)
    add("child_sat_n_65536", model=SAT_M, N=65536, K=0)
    add("child_perc_n_even", model=PERC_STEP_M, N=20, K=0)
    add("child_comm_k1_parity", model=COMM_STEP_M, N=28, K=7)
    return out


def probe(lib):
    lib = C.CDLL(lib._name)          # the same library under declarations of this file's own: device_ids may be NULL here
    lib.rrrmc_last_error.restype = C.c_char_p
    lib.rrrmc_last_error.argtypes = [C.c_void_p]
    res = {}
    for name, fn, null_out, a in cases():
        names, types, _ = SIGS[fn]
        f = getattr(lib, "rrrmc_ctx_" + fn)
        f.restype = C.c_int32
        f.argtypes = [C.POINTER(C.c_void_p)] + [t or C.POINTER(C.c_int32) for t in types]
        ctx = C.c_void_p()
        args = [a[n] if t else (None if a[n] is None else (C.c_int32 * len(a[n]))(*a[n])) for n, t in zip(names, types)]
        rc = f(None if null_out else C.byref(ctx), *args)
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
        assert "no HIP device" not in msg and "out of range (0.." not in msg, name      # (not the device query's)


if __name__ == "__main__":          # records the golden file: see the docstring
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as g
    with open(sys.argv[1], "w", encoding="utf-8") as fh:
        json.dump(probe(g.load_package().lib()), fh, indent=1, ensure_ascii=False, sort_keys=True)
        fh.write("\n")
