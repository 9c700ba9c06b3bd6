"""GraphCommQu beside GraphCommReLU at one shape on one device (profiles/r13/comm_qu.md): standardMC on the stand-alone graphs, rrrMC on
GraphCommQuRE / GraphCommReLURE in the LDS and thread builds, rrrMC and standardMC on GraphQCommQuT / GraphQCommReLUT in their three builds.
Kernel time from the device events around the sampler kernel (Engine.last_timing); per figure one warm-up call, then `--repeats` timed calls,
each from the configuration the last one left, the two machines alternating.  One JSON line per timed call; `--out FILE` also writes them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as e  # noqa: E402

SWITCHES = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS", "RRRMC_QUANT_NO_WAVE", "RRRMC_QUANT_NO_LDS", "RRRMC_QUANT_WAVE_MAX_R")

ap = argparse.ArgumentParser()
ap.add_argument("--k1", type=int, default=250)
ap.add_argument("--k2", type=int, default=4)
ap.add_argument("--p", type=int, default=400)
ap.add_argument("--m", type=int, default=5)
ap.add_argument("--beta", type=float, default=0.4)
ap.add_argument("--standalone", type=int, nargs="*", default=[8, 4096])
ap.add_argument("--ensemble", type=int, nargs="*", default=[8, 4096])
ap.add_argument("--quant", type=int, nargs="*", default=[8, 2048, 4096])
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()

pkg = e.load_package()
if pkg.lib().rrrmc_device_count() < 1:
    raise SystemExit("no HIP device: nothing is measured without one")
machines = {"Qu": pkg.GraphCommQu(a.k1, a.k2, a.p, seed=8370000274), "ReLU": pkg.GraphCommReLU(a.k1, a.k2, a.p, seed=8370000274)}
lines = []


def set_env(env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


def measure(family, graphs, R, sampler, build, env):
    """graphs: name -> graph; the engines alternate inside a repeat"""
    iters = 16384 if R <= 2048 else 4096
    set_env(env)
    engines = {}
    try:
        for name, X in graphs.items():
            eng = engines[name] = pkg.Engine(X, R)
            eng.seed(6540000789)
            eng.init_spins_random()
            (eng.rrr_mc if sampler == "rrrMC" else eng.standard_mc)(a.beta, 2048, 1024)          # warm-up at this shape
        for rep in range(a.repeats):
            for name, eng in engines.items():
                out = eng.rrr_mc(a.beta, iters, iters) if sampler == "rrrMC" else eng.standard_mc(a.beta, iters, iters)
                total_ms, kernel_ms, _ = eng.last_timing()
                rec = {"family": family, "machine": name, "shape": [a.k1, a.k2, a.p, a.m], "beta": a.beta, "sampler": sampler, "build": build,
                       "ran": eng.quant_pattern_build() if family == "quant" else None, "replicas": R, "repeat": rep, "iters_per_replica": iters,
                       "kernel_ms": kernel_ms, "call_ms": total_ms, "iterations_per_s": R * iters / (kernel_ms * 1e-3),
                       "acceptance": float(out[1].mean()) / iters}
                if sampler == "rrrMC":
                    rec["staged_share"] = float(out[2].mean()) / iters
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        for eng in engines.values():
            eng.close()
        set_env({})


for R in a.standalone:
    measure("standalone", machines, R, "standardMC", "thread", {})
re_graphs = {"Qu": pkg.GraphCommQuRE(machines["Qu"], a.m, 2.0, 0.4), "ReLU": pkg.GraphCommReLURE(machines["ReLU"], a.m, 2.0, 0.4)}
for R in a.ensemble:
    measure("re", re_graphs, R, "rrrMC", "lds", {"RRRMC_RE_LDS": "1"})
    measure("re", re_graphs, R, "rrrMC", "thread", {"RRRMC_RE_NO_LDS": "1"})
q_graphs = {"Qu": pkg.GraphQCommQuT(machines["Qu"], a.m, 0.3, 2.0), "ReLU": pkg.GraphQCommReLUT(machines["ReLU"], a.m, 0.3, 2.0)}
for R in a.quant:
    for build, env in (("lds", {"RRRMC_QUANT_WAVE_MAX_R": "1000000"}), ("wave-no-lds", {"RRRMC_QUANT_WAVE_MAX_R": "1000000", "RRRMC_QUANT_NO_LDS": "1"}),
                       ("thread", {"RRRMC_QUANT_NO_WAVE": "1"})):
        for sampler in ("rrrMC", "standardMC"):
            measure("quant", q_graphs, R, sampler, build, env)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
