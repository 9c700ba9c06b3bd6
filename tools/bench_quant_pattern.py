"""rrrMC / standardMC on GraphQPercStepT(Nk, P, M) against the closest existing path, GraphPercStepRE(Nk, P, M), at the same (Nk, P, M, R) on the
same device: the geometry of profiles/r08/perc.md (Nk = 1001, P = 400, M = 5), a handful of chains and a few thousand.  Kernel time from the
device events around the sampler kernel (Engine.last_timing); the two graphs alternate and every point is repeated, so that the spread is seen
next to the difference.  One JSON line per timed call; `--out FILE` also writes them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as e  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nk", type=int, default=1001)
ap.add_argument("--p", type=int, default=400)
ap.add_argument("--m", type=int, default=5)
ap.add_argument("--replicas", type=int, nargs="+", default=[8, 4096])
ap.add_argument("--iters", type=int, default=1 << 15)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()

pkg = e.load_package()
if pkg.lib().rrrmc_device_count() < 1:
    raise SystemExit("no HIP device: nothing is measured without one")
X1 = pkg.GraphPercStep(a.nk, a.p, seed=8370000274)
# the quantum graph at Γ = 0.3, β = 2 (fourK ≈ 2.1); the ensemble at γ = 2, graph β = 0.4 (profiles/r08/perc.md).  Sampler β = 0.4 for both,
# and the quantum graph also at its own β = 2, where it accepts about as often as the ensemble does at 0.4 and rrrMC takes the staged branch
Xq, Xre = pkg.GraphQPercStepT(X1, a.m, 0.3, 2.0), pkg.GraphPercStepRE(X1, a.m, 2.0, 0.4)
graphs = {"GraphQPercStepT": (Xq, 0.4), "GraphQPercStepT@beta=2": (Xq, 2.0), "GraphPercStepRE": (Xre, 0.4)}
lines = []
for R in a.replicas:
    engines = {}
    try:
        for name, (X, beta) in graphs.items():
            eng = engines[name] = pkg.Engine(X, R)
            eng.seed(6540000789)
            eng.init_spins_random()
            eng.rrr_mc(beta, 2048, 1024)                # warm-up of both kernels at this shape
            eng.standard_mc(beta, 2048, 1024)
        for rep in range(a.repeats):
            for sampler in ("rrrMC", "standardMC"):
                for name, eng in engines.items():       # alternate the two graphs inside a repeat
                    beta = graphs[name][1]
                    out = eng.rrr_mc(beta, a.iters, a.iters) if sampler == "rrrMC" else eng.standard_mc(beta, a.iters, a.iters)
                    total_ms, kernel_ms, _ = eng.last_timing()
                    rec = {"graph": "%s(%d, %d, %d)" % (name.split("@")[0], a.nk, a.p, a.m), "beta": beta, "sampler": sampler, "replicas": R, "repeat": rep,
                           "build": eng.quant_pattern_build() if name.startswith("GraphQ") else None,
                           "iters_per_replica": a.iters, "kernel_ms": kernel_ms, "call_ms": total_ms,
                           "iterations_per_s": R * a.iters / (kernel_ms * 1e-3), "acceptance": float(out[1].mean()) / a.iters}
                    if sampler == "rrrMC":
                        rec["staged_share"] = float(out[2].mean()) / a.iters
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
    finally:
        for eng in engines.values():
            eng.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
