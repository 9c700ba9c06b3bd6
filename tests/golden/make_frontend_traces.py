#!/usr/bin/env python3
"""Write tests/golden/frontend_traces.json: what the Python front end (rrrmc.jl_amd/engine.py, graphs.py) asks of the C ABI, call by call.

The library is replaced by a recording stand-in (``Recorder``): the host-only functions (generators, discretize, tables) run for real, every
call that takes a context is written down (its name less the ``rrrmc_``) — scalars as they are, arrays as dtype, shape and crc32 of their bytes, raw pointers as ``ptr`` —
and answered with status 0 and deterministic output.  No device is needed.  The cases: creating, uploading and closing an ``Engine`` for every
graph family on one device and on two, an upload that fails, the ``Engine`` methods that depend on the family, and the five sampler functions
with and without hooks (what each hook call saw, what came back, what was printed).  Replayed by tests/test_frontend_trace_cpu.py.

  python tests/golden/make_frontend_traces.py      (from the repo root)"""
import contextlib
import ctypes as C
import io
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "frontend_traces.json")

HOST_ONLY = ("rrrmc_gen_", "rrrmc_discretize", "rrrmc_re_tables", "rrrmc_le_tables", "rrrmc_version")
# array arguments the library writes (position in the call); every other array is an input
OUTPUTS = {"rrrmc_get_spins": (1,), "rrrmc_energy": (1,), "rrrmc_energy_f64": (1,), "rrrmc_get_fields": (1,), "rrrmc_get_fields_f64": (1,),
           "rrrmc_tracked_energy": (1,), "rrrmc_tracked_energy_f64": (1,), "rrrmc_rrr_stats": (1,), "rrrmc_wtm_times": (1,),
           "rrrmc_extremal_opt_results": (1, 2, 3), "rrrmc_extremal_opt_results_f64": (1, 2, 3), "rrrmc_re_energies": (1,),
           "rrrmc_le_energies": (1,), "rrrmc_le_cenergy": (1,), "rrrmc_le_distances": (1,), "rrrmc_snapshot_get": (2,)}
# sampling calls: position of (iters, step); rrrmc_results_samples then answers iters // step (wtmMC: its `samples`)
SAMPLING = {"rrrmc_standard_mc": (2, 3), "rrrmc_standard_mc_f64": (2, 3), "rrrmc_standard_mc_async": (2, 3), "rrrmc_standard_mc_fast_async": (2, 3),
            "rrrmc_colored_sweeps_async": (2, 3), "rrrmc_rrr_mc_async": (3, 4), "rrrmc_bkl_mc_async": (2, 3), "rrrmc_wtm_mc_async": (2, None),
            "rrrmc_extremal_opt_async": (2, 3)}


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def pattern(k, n, dtype):
    """the deterministic content of the k-th call's output of n elements"""
    return ((k * 2654435761 + np.arange(n, dtype=np.uint64) * 40503) % 251).astype(dtype)


def describe(v):
    """a result in JSON terms: type, dtype and shape or length, crc32"""
    if isinstance(v, np.ndarray):
        return "ndarray %s%s#%08x" % (v.dtype.str, list(v.shape), crc(v))
    if isinstance(v, (list, tuple)):
        return [type(v).__name__] + [describe(x) for x in v]
    if hasattr(v, "s") and hasattr(v, "R"):
        return "Config(%d, %d)#%08x" % (v.N, v.R, crc(v.s))
    if isinstance(v, np.generic):
        return "%s %r" % (type(v).__name__, v.item())
    return v


class Recorder:
    """Stands in for the loaded library (the module global ``_lib._lib``)."""

    def __init__(self, real):
        self.real = real
        self.calls = []
        self.index = 0              # of the call, over the recorder's life: seeds the output patterns
        self.R = 0                  # replicas of the last context made
        self.nsamp = 0              # iters // step of the last sampling call
        self.fail_next_set = 0      # status the next rrrmc_set_* call returns

    def take(self):
        calls, self.calls = self.calls, []
        return calls

    def __getattr__(self, name):
        if name.startswith(HOST_ONLY):
            return getattr(self.real, name)
        if name == "rrrmc_last_error":
            return lambda ctx=None: self.real.rrrmc_last_error(None)        # the stand-in's contexts are not the library's
        fn = getattr(self.real, name)                                       # an unknown symbol is an AttributeError, as with the library
        return lambda *a: self._call(name, fn.argtypes, a)

    def _call(self, name, argtypes, args):
        assert argtypes is None or len(argtypes) == len(args), "%s takes %d arguments, given %d" % (name, len(argtypes), len(args))
        self.index += 1
        out = []
        for i, x in enumerate(args):
            t = argtypes[i] if argtypes else None
            if isinstance(x, np.ndarray):
                t.from_param(x)                                             # dtype and contiguity, as ctypes would check them
                out.append("%s%s#%08x" % (x.dtype.str, list(x.shape), crc(x)))
                if i in OUTPUTS.get(name, ()):
                    x.reshape(-1)[:] = pattern(self.index, x.size, x.dtype)
            elif hasattr(x, "_obj"):                                        # byref(...)
                out.append("ref")
                if name.startswith("rrrmc_ctx_create"):
                    x._obj.value = 1
            elif t is C.c_void_p:
                out.append("ctx" if isinstance(x, C.c_void_p) else "None" if x is None else "ptr")
            else:
                out.append(repr(x.item() if isinstance(x, np.generic) else x))
        self.calls.append("%s(%s)" % (name[len("rrrmc_"):], ", ".join(out)))
        if name.startswith("rrrmc_ctx_create"):
            self.R = int(args[-4] if name == "rrrmc_ctx_create_multi" else args[-3])
        if name in SAMPLING:
            it, st = SAMPLING[name]
            self.nsamp = int(args[it]) // int(args[st]) if st is not None else int(args[it])
        if name in ("rrrmc_standard_mc", "rrrmc_standard_mc_f64", "rrrmc_fetch_results", "rrrmc_fetch_results_f64"):
            Es, acc = args[-2], args[-1]
            if Es is not None:
                et = C.c_double if name.endswith("_f64") else C.c_int64
                (et * (self.R * self.nsamp)).from_address(Es)[:] = pattern(self.index, self.R * self.nsamp, np.int64).tolist()
            (C.c_int64 * self.R).from_address(acc)[:] = pattern(self.index + 500009, self.R, np.int64).tolist()
        if name == "rrrmc_results_samples":
            return self.nsamp
        if name.startswith("rrrmc_set_") and self.fail_next_set and name not in ("rrrmc_set_resume", "rrrmc_set_spins"):
            rc, self.fail_next_set = self.fail_next_set, 0
            return rc
        return 0


def graph_cases(pkg):
    """name -> constructor, one per branch of the create / upload code, at the smallest shapes the constructors accept"""
    g, b = 0.5, 2.0
    slices = [("empty", lambda: None, 5), ("sk", lambda: pkg.GraphSK(8), 8), ("skn", lambda: pkg.GraphSKNormal(8), 8),
              ("percstep", lambda: pkg.GraphPercStep(11, 5), 11), ("perclinear", lambda: pkg.GraphPercLinear(11, 5), 11),
              ("commstep", lambda: pkg.GraphCommStep(3, 3, 5), 9), ("commrelu", lambda: pkg.GraphCommReLU(4, 2, 5), 8)]
    cases = {
        "rrg": lambda: pkg.GraphRRG(10, 3),
        "ea": lambda: pkg.GraphEA(2, 2),
        "rrg-levels": lambda: pkg.GraphRRG(10, 3, LEV=(-1, 0, 1)),
        "rrg-k8": lambda: pkg.GraphRRG(20, 8, seed=324),       # K > PM1_MAX_K: the levels route; a seed whose pairing gives a simple graph
        "ea-levels": lambda: pkg.GraphEA(2, 2, LEV=(-1.5, 0.5)),
        "rrg-normal": lambda: pkg.GraphRRGNormal(10, 3),
        "ea-normal": lambda: pkg.GraphEANormal(3, 2),
        "rrg-discretized": lambda: pkg.GraphRRGNormalDiscretized(10, 3, (-1, 0, 1)),
        "ea-discretized": lambda: pkg.GraphEANormalDiscretized(3, 2, (-1.5, 0.0, 1.5)),
        "sk-normal": lambda: pkg.GraphSKNormal(8),
        "sk": lambda: pkg.GraphSK(8),
        "quant-rrg": lambda: pkg.GraphQuant(pkg.GraphRRG(10, 3), 4, 0.3, b),
        "quant-ea": lambda: pkg.GraphQuant(pkg.GraphEA(2, 2), 4, 0.3, b),
        "quant-sk": lambda: pkg.GraphQuant(pkg.GraphSK(8), 4, 0.3, b),
        "quant-skn": lambda: pkg.GraphQuant(pkg.GraphSKNormal(8), 4, 0.3, b),
        "quant-qeat": lambda: pkg.GraphQEAT(2, 2, 4, 0.3, b),
        "perc-step": lambda: pkg.GraphPercStep(11, 5),
        "perc-linear": lambda: pkg.GraphPercLinear(11, 5),
        "comm-step": lambda: pkg.GraphCommStep(3, 3, 5),
        "comm-relu": lambda: pkg.GraphCommReLU(4, 2, 5),
    }
    for ens, E in (("re", pkg.GraphRobustEnsemble), ("le", pkg.GraphLocalEntropy)):
        for name, make, Nk in slices:
            cases["%s-%s" % (ens, name)] = (lambda E=E, make=make, Nk=Nk: E(Nk, 3, g, b, make()))
    return cases


def engine_trace(pkg, rec, X, **kw):
    eng = pkg.Engine(X, 2, **kw)
    linked = getattr(X, "_engine", None) is eng
    eng.close()
    return {"calls": rec.take(), "graph_engine_link": [linked, getattr(X, "_engine", None) is None]}


def failing_upload(pkg, rec, X, **kw):
    rec.fail_next_set = 3
    try:
        pkg.Engine(X, 2, **kw)
        raised = None
    except pkg.RRRMCError as e:
        raised = e.code
    rec.fail_next_set = 0
    return {"calls": rec.take(), "raised": raised, "graph_engine_unlinked": getattr(X, "_engine", None) is None}


def method_cases(pkg):
    g, b = 0.5, 2.0
    return {
        "rrg": lambda: pkg.GraphRRG(10, 3),
        "rrg-levels": lambda: pkg.GraphRRG(10, 3, LEV=(-1, 0, 1)),
        "ea-levels-float": lambda: pkg.GraphEA(2, 2, LEV=(-1.5, 0.5)),
        "sk": lambda: pkg.GraphSK(8),
        "sk-normal": lambda: pkg.GraphSKNormal(8),
        "rrg-normal": lambda: pkg.GraphRRGNormal(10, 3),
        "rrg-discretized": lambda: pkg.GraphRRGNormalDiscretized(10, 3, (-1, 0, 1)),
        "perc-step": lambda: pkg.GraphPercStep(11, 5),
        "perc-linear": lambda: pkg.GraphPercLinear(11, 5),
        "comm-relu": lambda: pkg.GraphCommReLU(4, 2, 5),
        "quant-rrg": lambda: pkg.GraphQuant(pkg.GraphRRG(10, 3), 4, 0.3, b),
        "quant-sk": lambda: pkg.GraphQuant(pkg.GraphSK(8), 4, 0.3, b),
        "re-m4": lambda: pkg.GraphSKRE(8, 4, g, b),
        "re-m5": lambda: pkg.Graph0RE(5, 5, g, b),
        "le-m4": lambda: pkg.GraphSKLE(8, 4, g, b),
        "le-m5": lambda: pkg.Graph0LE(5, 5, g, b),
    }


def method_trace(pkg, rec, X):
    res = {}
    with pkg.Engine(X, 2) as eng:
        res["energy"] = describe(eng.energy())
        res["fields"] = describe(eng.fields())
        res["rrr_mc"] = describe(eng.rrr_mc(1.0, 20, 10, staged_thr=None))
        res["rrr_cache"] = describe(eng.rrr_cache())
        res["tracked_energy"] = describe(eng.tracked_energy())
        res["run_energy"] = describe(eng.run_energy())
    return {"calls": rec.take(), "returned": res}


class Hook:
    """``hook(it, X, C, a, b)`` of the five samplers; ``answer(n)`` = what the n-th call (from 1) returns, or raises"""

    def __init__(self, answer):
        self.answer, self.seen = answer, []

    def __call__(self, it, X, Cfg, a, b):
        self.seen.append([it, describe(Cfg.s), describe(a), describe(b)])
        return self.answer(len(self.seen))


class HookError(Exception):
    pass


def _raise(n):
    if n >= 2:
        raise HookError("the hook's own failure")
    return True


ANSWERS = {
    "continue": lambda n: True,
    "stop-at-2": lambda n: n < 2,
    "freeze-1-at-2": lambda n: np.array([True, n < 2, True]),
    "freeze-all": lambda n: np.array([n < 1, n < 2, n < 2]),           # replica 0 at the first call, the others at the second
    "raise-at-2": _raise,
}


def sampler_cases(pkg):
    """name -> (graph, function, first positional arguments, (long run, short run with step > iters, run that ends on a sample))"""
    rrg, rrgn = (lambda: pkg.GraphRRG(10, 3)), (lambda: pkg.GraphRRGNormal(10, 3))
    runs = ((35, 10), (5, 10), (30, 10))
    return {
        "standardMC": (rrg, pkg.standardMC, 1.0, runs),
        "standardMC-f64": (rrgn, pkg.standardMC, 1.0, runs),
        "rrrMC": (rrg, pkg.rrrMC, 1.0, runs),
        "bklMC": (rrg, pkg.bklMC, 1.0, runs),
        "wtmMC": (rrg, pkg.wtmMC, 1.0, ((4, 1.0), (1, 2.5), (3, 0.5))),
        "extremal_opt": (rrg, pkg.extremal_opt, 1.3, runs),
    }


def sampler_trace(pkg, rec, make, fn, par, run, answer=None, engine=False, C0=False, quiet=False):
    X = make()
    hook = Hook(ANSWERS[answer]) if answer else None
    kw = {"step": run[1], "hook": hook, "quiet": quiet}
    eng = c0 = None
    if engine:
        eng = kw["engine"] = pkg.Engine(X, 3)
        kw["seed"] = 0
    if C0:
        c0 = kw["C0"] = pkg.Config(X.N, 3, pattern(7, 3, np.uint64).reshape(3, 1))
    if not engine and not C0:
        kw["replicas"] = 3
    res = {}
    stdout = io.StringIO()
    try:
        with contextlib.redirect_stdout(stdout):
            ret = fn(X, par, run[0], **kw)
        res["returned"] = describe(ret)
        if c0 is not None:
            res["C0_is_returned"] = any(r is c0 for r in ret)
    except HookError as e:
        res["raised"] = str(e)
    finally:
        if eng is not None:
            eng.close()
    res["calls"] = rec.take()
    res["hook"] = hook.seen if hook else None
    res["stdout"] = stdout.getvalue()
    if c0 is not None:
        res["C0"] = describe(c0)
    return res


def generate(pkg, rec):
    """every case -> what was recorded; ``rec`` must already stand in for the library"""
    out = {}
    for name, make in graph_cases(pkg).items():
        out["engine/%s" % name] = engine_trace(pkg, rec, make())
        out["engine-2dev/%s" % name] = engine_trace(pkg, rec, make(), devices=[0, 1])
    G = graph_cases(pkg)
    for name in ("rrg", "rrg-levels", "quant-ea", "re-sk", "le-commrelu"):
        out["upload-fails/%s" % name] = failing_upload(pkg, rec, G[name]())
    out["upload-fails-2dev/quant-sk"] = failing_upload(pkg, rec, G["quant-sk"](), devices=[0, 1])
    for name, make in method_cases(pkg).items():
        out["methods/%s" % name] = method_trace(pkg, rec, make())
    for name, (make, fn, par, (long, short, exact)) in sampler_cases(pkg).items():
        def case(tag, run, **kw):
            out["%s/%s" % (name, tag)] = sampler_trace(pkg, rec, make, fn, par, run, **kw)
        case("no-hook", long)
        for answer in ANSWERS if name != "standardMC-f64" else ("continue", "freeze-1-at-2", "raise-at-2"):
            case(answer, long, answer=answer)
        case("step-beyond-iters-continue", short, answer="continue")
        if name == "standardMC-f64":            # the same code as standardMC but for the opening call: the variants that reach it differently
            continue
        case("engine-seed0-quiet", long, engine=True, quiet=True)
        case("engine-seed0-freeze-1-at-2", long, answer="freeze-1-at-2", engine=True)
        case("engine-seed0-raise-at-2", long, answer="raise-at-2", engine=True)
        case("C0", long, C0=True)
        case("engine-C0-freeze-all", long, answer="freeze-all", engine=True, C0=True)
        case("step-beyond-iters", short)
        case("ends-on-a-sample-freeze-1-at-2", exact, answer="freeze-1-at-2")
    return out


def load():
    """(package, its _lib module, a Recorder over the real library)"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    L = sys.modules[pkg.__name__ + "._lib"]
    return pkg, L, Recorder(pkg.lib())


def main():
    pkg, L, rec = load()
    real, L._lib = L._lib, rec
    try:
        out = generate(pkg, rec)
    finally:
        L._lib = real
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
