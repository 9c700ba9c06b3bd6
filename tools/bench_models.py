#!/usr/bin/env python3
"""Secondary benchmarks (not the headline metric): throughput of the other model kernels on one GPU.
  python tools/bench_models.py sk      GraphSKNormal N=1024, 2048 replicas (BASELINE.json configs[2])
  python tools/bench_models.py re [R ...]   GraphSKRE(1024, 5), γ = 2, β = 0.4: rrrMC (both builds) and standardMC
  python tools/bench_models.py le [R ...]   GraphSKLE(1024, 5), γ = 2, β = 0.4: rrrMC (both builds) and standardMC
  python tools/bench_models.py perc [R ...] GraphPercStepRE / GraphPercStepLE(1001, 400, 5) and GraphPercStep(1001, 400): the same three legs
  python tools/bench_models.py comm [R ...] GraphCommStepRE / LE(201, 5, 400, 5), GraphCommReLURE / LE(168, 6, 400, 5) and the two
                                            stand-alone graphs: the same legs
  python tools/bench_models.py sat [R ...]  GraphSAT(1000, 3, 4.2), β = 2: standardMC through the wave and the thread build
  python tools/bench_models.py tle [R ...]  GraphSATTLE(1000, 3, 4.2, 3) and GraphSKTLE(201, 3) beside LE: rrrMC (both builds) and standardMC
  python tools/bench_models.py satre [R ...] GraphSATRE(1001, 3, 4.2, 5) beside GraphPercStepRE(1001, 400, 5): rrrMC, both builds
  python tools/bench_models.py xentr [R ...] GraphPercXEntr(1001, 400, 1.0), β = 1: standardMC through the wave and the thread build, the table in
                                            LDS and in global memory, beside GraphPercLinear(1001, 400)
  python tools/bench_models.py eare [R ...] GraphEARE / GraphEATLE(10, 3, 5) at β = 0.8 and 0.2 beside GraphSKRE(1024, 5): rrrMC (both builds)
                                            and standardMC
  python tools/bench_models.py mixed [R ...] GraphMixed(GraphSK(1001), GraphPercStep(1001, 400), GraphSAT(1001, 3, 4.2)), β = 1: standardMC through
                                            the wave and the thread build, and rrrMC through GraphAddSubFields over it
  python tools/bench_models.py pspin3 [R ...] GraphPSpin3(3000, 3) and GraphPSpin3(3000, 8), β = 1: standardMC through the wave and the thread build,
                                            beside GraphSAT(3000, 3, 4.2) under the same call
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def bench_sk(N=1024, R=2048, beta=1.0, iters=1 << 16, step=1 << 10, seed=0x5EED):
    if len(sys.argv) > 2:                                    # python tools/bench_models.py sk N [R] [binary]
        N = int(sys.argv[2]); R = int(sys.argv[3]) if len(sys.argv) > 3 else R
    binary = len(sys.argv) > 4 and sys.argv[4] == "binary"
    pkg = entry.load_package()
    X = pkg.GraphSK(N, seed=seed) if binary else pkg.GraphSKNormal(N, seed=seed)
    eng = pkg.Engine(X, R)
    eng.seed(seed)
    eng.init_spins_random()
    eng.standard_mc_async(beta, iters // 4, step); eng.sync()
    t0 = time.perf_counter()
    eng.standard_mc_async(beta, iters, step); eng.sync()
    dt = time.perf_counter() - t0
    total_ms, sweep_ms, _ = eng.last_timing()
    Es, acc = eng.fetch_results()
    a = float(acc.mean()) / iters
    attempts = float(R) * iters
    bytes_per_attempt = 8 + a * (17 * N + 2)                 # SURVEY.md §8d, dense SK Float64
    out = {"model": "GraphSK" if binary else "GraphSKNormal", "N": N, "replicas": R, "beta": beta, "iters": iters, "attempts_per_s": attempts / dt,
           "kernel_ms": sweep_ms, "acceptance": a, "energy_per_spin": float(Es[:, -1].mean()) / N,
           "algorithmic_bytes_per_attempt": bytes_per_attempt,
           "algorithmic_GBps_kernel": bytes_per_attempt * attempts / (sweep_ms * 1e-3) / 1e9}
    print(json.dumps(out))
    eng.close()


def bench_ea(L=64, D=3, R=512, beta=1.0, sweeps=64, step=16, seed=0x5EED):
    """BASELINE.json configs[3] on ONE GPU's share: GraphEA L=64 D=3, 512 of the 4096 replicas, checkerboard sweeps."""
    pkg = entry.load_package()
    X = pkg.GraphEA(L, D, seed=seed)
    eng = pkg.Engine(X, R)
    eng.seed(seed)
    eng.init_spins_random()
    eng.set_coloring(pkg.checkerboard_coloring(L, D))
    eng.colored_sweeps_async(beta, 8, 8); eng.sync()
    t0 = time.perf_counter()
    eng.colored_sweeps_async(beta, sweeps, step); eng.sync()
    dt = time.perf_counter() - t0
    total_ms, sweep_ms, _ = eng.last_timing()
    Es, _ = eng.fetch_results()
    attempts = float(R) * sweeps * X.N
    out = {"model": "GraphEA checkerboard", "L": L, "D": D, "replicas": R, "beta": beta, "sweeps": sweeps,
           "attempts_per_s": attempts / dt, "device_ms": sweep_ms, "energy_per_spin": float(Es[:, -1].mean()) / X.N}
    print(json.dumps(out))
    eng.close()


def bench_quant(Nk=1024, M=32, R=128, beta=2.0, Gamma=0.5, iters=1 << 16, step=1 << 12, seed=0x5EED):
    """BASELINE.json configs[4] on ONE GPU's share: GraphQuant(GraphRRG(1024,3), M=32) under rrrMC, 128 of the 1024 replicas."""
    pkg = entry.load_package()
    X = pkg.GraphQuant(pkg.GraphRRG(Nk, 3, seed=seed), M, Gamma, beta)
    for R in ([int(a) for a in sys.argv[2:]] or [R]):        # the path scales with the replicas: python tools/bench_models.py quant 128 1024 8192
        it = max(step, iters * 128 // max(R, 128))
        eng = pkg.Engine(X, R)
        eng.seed(seed)
        eng.init_spins_random()
        t0 = time.perf_counter()
        Es, acc, staged = eng.rrr_mc(beta, it, step)
        dt = time.perf_counter() - t0
        total_ms, sweep_ms, _ = eng.last_timing()
        out = {"model": "GraphQuant rrrMC", "Nk": Nk, "M": M, "replicas": R, "beta": beta, "Gamma": Gamma, "iters": it,
               "iterations_per_s": float(R) * it / dt, "kernel_iterations_per_s": float(R) * it / (sweep_ms * 1e-3), "kernel_ms": sweep_ms,
               "acceptance": float(acc.mean()) / it, "staged_frac": float(staged.mean()) / it, "energy_per_spin": float(Es[:, -1].mean()) / X.N}
        print(json.dumps(out), flush=True)
        eng.close()


def bench_spf(N=4096, K=3, R=65536, beta=1.0, iters=1 << 16, step=1 << 12, seed=0x5EED):
    """GraphRRGNormal (Float64 sparse): config-2 geometry with Gaussian couplings; the lane-per-replica
    kernel hides its accept-path latency with occupancy, so it is measured at several replica counts."""
    pkg = entry.load_package()
    K = int(os.environ.get("BENCH_SPF_K", K))            # (K = 7, 8: the degrees without fused pairs)
    X = pkg.GraphRRGNormal(N, K, seed=seed)
    model = "GraphRRGNormal"
    if os.environ.get("BENCH_SPF_EA"):                   # "L,D": GraphEANormal(L, D) instead (K = 2 D; L = 8, D = 4 has the N of the default)
        L_, D_ = (int(a) for a in os.environ["BENCH_SPF_EA"].split(","))
        X = pkg.GraphEANormal(L_, D_, seed=seed)
        N, K, model = X.N, 2 * D_, "GraphEANormal(L=%d,D=%d)" % (L_, D_)
    for R in ([int(a) for a in sys.argv[2:]] or [8192, 65536, 262144]):
        eng = pkg.Engine(X, R)
        eng.seed(seed)
        eng.init_spins_random()
        eng.standard_mc_async(beta, iters // 4, step); eng.sync()
        t0 = time.perf_counter()
        eng.standard_mc_async(beta, iters, step); eng.sync()
        dt = time.perf_counter() - t0
        total_ms, sweep_ms, _ = eng.last_timing()
        Es, acc = eng.fetch_results()
        a = float(acc.mean()) / iters
        attempts = float(R) * iters
        bpa = 8 + a * (10 + 17 * K)          # SURVEY.md §8d widths: field 8 B, spin 1 B; lfields_last excluded
        out = {"model": model, "N": N, "K": K, "replicas": R, "beta": beta, "iters": iters, "attempts_per_s": attempts / dt,
               "build": {k: os.environ[k] for k in ("RRRMC_SPF_TEAM", "RRRMC_SPF_TEAM_WAVES", "RRRMC_SPF_TEAM_WIDTH") if k in os.environ} or "default",
               "kernel_ms": sweep_ms, "acceptance": a, "energy_per_spin": float(Es[:, -1].mean()) / N,
               "algorithmic_bytes_per_attempt": bpa, "algorithmic_GBps_kernel": bpa * attempts / (sweep_ms * 1e-3) / 1e9}
        print(json.dumps(out), flush=True)
        eng.close()


def bench_spf_fast(N=4096, K=3, beta=1.0, iters=1 << 20, step=1 << 12, seed=0x5EED):
    """GraphRRGNormal under the opt-in fast standardMC (bit-sliced replicas, per-site thresholds): python tools/bench_models.py spf_fast 8192"""
    pkg = entry.load_package()
    X = pkg.GraphRRGNormal(N, K, seed=seed)
    for R in ([int(a) for a in sys.argv[2:]] or [8192]):
        for st in (step, 16 * step):
            eng = pkg.Engine(X, R)
            eng.seed(seed)
            eng.init_spins_random()
            eng.standard_mc_fast_async(beta, iters, st); eng.sync()      # warm-up of the same shape (buffers, chunk list, thresholds)
            t0 = time.perf_counter()
            eng.standard_mc_fast_async(beta, iters, st); eng.sync()
            dt = time.perf_counter() - t0
            total_ms, sweep_ms, nl = eng.last_timing()
            Es, acc = eng.fetch_results()
            a = float(acc.mean()) / iters
            attempts = float(R) * iters
            bpa = 8 + a * (10 + 17 * K)
            print(json.dumps({"model": "GraphRRGNormal fast standardMC", "N": N, "K": K, "replicas": R, "beta": beta, "iters": iters, "step": st,
                              "attempts_per_s": attempts / dt, "kernel_ms": sweep_ms, "launches": nl, "acceptance": a,
                              "energy_per_spin": float(Es[:, -1].mean()) / N, "algorithmic_bytes_per_attempt": bpa,
                              "algorithmic_GBps_kernel": bpa * attempts / (sweep_ms * 1e-3) / 1e9}), flush=True)
            eng.close()


def bench_dbl(N=4096, K=3, R=8192, beta=2.0, iters=1 << 14, step=1 << 12, seed=0x5EED):
    """GraphRRGNormalDiscretized(N, K, (-1,0,1)) under rrrMC(X::DoubleGraph): thread-per-replica kernel."""
    pkg = entry.load_package()
    X = pkg.GraphRRGNormalDiscretized(N, K, (-1, 0, 1), seed=seed)
    for R in ([int(a) for a in sys.argv[2:]] or [R]):
        eng = pkg.Engine(X, R)
        eng.seed(seed)
        eng.init_spins_random()
        t0 = time.perf_counter()
        Es, acc, staged = eng.rrr_mc(beta, iters, step)
        dt = time.perf_counter() - t0
        total_ms, sweep_ms, _ = eng.last_timing()
        out = {"model": "GraphRRGNormalDiscretized rrrMC", "N": N, "K": K, "replicas": R, "beta": beta, "iters": iters,
               "iterations_per_s": float(R) * iters / dt, "kernel_ms": sweep_ms, "acceptance": float(acc.mean()) / iters,
               "staged_frac": float(staged.mean()) / iters, "energy_per_spin": float(Es[:, -1].mean()) / X.N}
        print(json.dumps(out), flush=True)
        eng.close()


def bench_ea_random(L=64, D=3, beta=1.0, sweeps=8, seed=0x5EED):
    """GraphEA(64, 3) (BASELINE.json configs[3]'s lattice, N = 262 144) under the reference's own random-site standardMC: the big-N
    kernels (spins in HBM/L2).  python tools/bench_models.py ea_random 512 4096"""
    pkg = entry.load_package()
    X = pkg.GraphEA(L, D, seed=seed)
    for R in ([int(a) for a in sys.argv[2:]] or [512, 4096]):
        eng = pkg.Engine(X, R)
        eng.seed(seed)
        eng.init_spins_random()
        iters = sweeps * X.N
        eng.standard_mc_async(beta, X.N, X.N); eng.sync()
        t0 = time.perf_counter()
        eng.standard_mc_async(beta, iters, X.N); eng.sync()
        dt = time.perf_counter() - t0
        total_ms, sweep_ms, nl = eng.last_timing()
        Es, acc = eng.fetch_results()
        print(json.dumps({"model": "GraphEA random-site standardMC (big-N kernels)", "L": L, "D": D, "replicas": R, "beta": beta,
                          "iters": iters, "attempts_per_s": float(R) * iters / dt, "sweep_kernel_ms": sweep_ms, "launches": nl,
                          "acceptance": float(acc.mean()) / iters, "energy_per_spin": float(Es[:, -1].mean()) / X.N}), flush=True)
        eng.close()


def bench_re(Nk=1024, M=5, gamma=2.0, beta=0.4, iters=1 << 14, step=1 << 12, seed=0x5EED):
    """GraphSKRE(1024, 5), γ = 2, β = 0.4 (scripts.jl:866-963 test_REIsing): rrrMC through the thread and the LDS build and standardMC, kernel
    iterations/s per replica count (python tools/bench_models.py re 128 1024 4096), and the standardMC-per-rrrMC time ratio of the pair."""
    pkg = entry.load_package()
    X = pkg.GraphSKRE(Nk, M, gamma, beta, seed=seed)
    for R in ([int(a) for a in sys.argv[2:]] or [128, 1024, 4096]):
        it = max(step, iters * 1024 // max(R, 1024))
        out = {"model": "GraphSKRE", "Nk": Nk, "M": M, "gamma": gamma, "beta": beta, "replicas": R, "iters": it}
        for name, env in (("rrr_thread", {"RRRMC_RE_NO_LDS": "1"}), ("rrr_lds", {"RRRMC_RE_LDS": "1"}), ("standard", {})):
            for k in ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS"):
                os.environ.pop(k, None)
            os.environ.update(env)
            eng = pkg.Engine(X, R)
            eng.seed(seed)
            eng.init_spins_random()
            if name == "standard":
                eng.standard_mc(beta, it, step)                  # warm-up, then the timed call from the configuration it left
                Es, acc = eng.standard_mc(beta, it, step)
                staged = np.zeros(R)
            else:
                eng.rrr_mc(beta, it, step)
                Es, acc, staged = eng.rrr_mc(beta, it, step)
            _, sweep_ms, _ = eng.last_timing()
            out[name] = {"kernel_iterations_per_s": float(R) * it / (sweep_ms * 1e-3), "kernel_ms": sweep_ms,
                         "acceptance": float(acc.mean()) / it, "staged_frac": float(staged.mean()) / it,
                         "energy_per_spin": float(Es[:, -1].mean()) / X.N}
            eng.close()
        for k in ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS"):
            os.environ.pop(k, None)
        best = max(out["rrr_thread"]["kernel_iterations_per_s"], out["rrr_lds"]["kernel_iterations_per_s"])
        # seconds of standardMC per second of rrrMC at met_factor standardMC iterations per rrrMC iteration (scripts.jl:877: 20.8)
        out["met_factor_time_ratio"] = 20.8 * best / out["standard"]["kernel_iterations_per_s"]
        out["iters_ratio_equal_time"] = out["standard"]["kernel_iterations_per_s"] / best
        print(json.dumps(out), flush=True)


def bench_le(Nk=1024, M=5, gamma=2.0, beta=0.4, iters=1 << 14, step=1 << 12, seed=0x5EED):
    """GraphSKLE(1024, 5), γ = 2, β = 0.4 (bench_re's point, with the explicit centre: N = 1024 * 6): rrrMC through the thread and the LDS build
    and standardMC, kernel iterations/s per replica count (python tools/bench_models.py le 128 1024 4096)."""
    pkg = entry.load_package()
    X = pkg.GraphSKLE(Nk, M, gamma, beta, seed=seed)
    envs = ("RRRMC_LE_NO_LDS", "RRRMC_LE_LDS")
    for R in ([int(a) for a in sys.argv[2:]] or [128, 1024, 4096]):
        it = max(step, iters * 1024 // max(R, 1024))
        out = {"model": "GraphSKLE", "Nk": Nk, "M": M, "gamma": gamma, "beta": beta, "replicas": R, "iters": it}
        for name, env in (("rrr_thread", {"RRRMC_LE_NO_LDS": "1"}), ("rrr_lds", {"RRRMC_LE_LDS": "1"}), ("standard", {})):
            for k in envs:
                os.environ.pop(k, None)
            os.environ.update(env)
            eng = pkg.Engine(X, R)
            eng.seed(seed)
            eng.init_spins_random()
            if name == "standard":
                eng.standard_mc(beta, it, step)                  # warm-up, then the timed call from the configuration it left
                Es, acc = eng.standard_mc(beta, it, step)
                staged = np.zeros(R)
            else:
                eng.rrr_mc(beta, it, step)
                Es, acc, staged = eng.rrr_mc(beta, it, step)
            _, sweep_ms, _ = eng.last_timing()
            out[name] = {"kernel_iterations_per_s": float(R) * it / (sweep_ms * 1e-3), "kernel_ms": sweep_ms,
                         "acceptance": float(acc.mean()) / it, "staged_frac": float(staged.mean()) / it,
                         "energy_per_spin": float(Es[:, -1].mean()) / X.N}
            eng.close()
        for k in envs:
            os.environ.pop(k, None)
        best = max(out["rrr_thread"]["kernel_iterations_per_s"], out["rrr_lds"]["kernel_iterations_per_s"])
        out["iters_ratio_equal_time"] = out["standard"]["kernel_iterations_per_s"] / best
        print(json.dumps(out), flush=True)


def bench_tle(M=3, gamma=1.0, lam=0.5, beta_g=1.0, beta=1.0, iters=10000, seed=7):
    """GraphSATTLE(1000, 3, 4.2, 3) and GraphSKTLE(201, 3) (γ = 1, λ = 0.5, β = 1) beside GraphSATLE / GraphSKLE at the same shape: rrrMC
    through TLE's LDS and global-memory builds and standardMC, kernel iterations/s per replica count (python tools/bench_models.py tle 8
    128 2048; profiles/r14/tle.md).  Every figure: one warm-up call, then two timed calls continuing the chain, the faster one reported."""
    pkg = entry.load_package()
    S = pkg.GraphSAT(1000, 3, 4.2, seed=seed)
    models = (("GraphSATTLE(1000,3,4.2,%d)" % M, pkg.GraphSATTLE(S, M, gamma, lam, beta_g), pkg.GraphSATLE(S, M, gamma, beta_g)),
              ("GraphSKTLE(201,%d)" % M, pkg.GraphSKTLE(201, M, gamma, lam, beta_g, seed=seed), pkg.GraphSKLE(201, M, gamma, beta_g, seed=seed)))
    envs = ("RRRMC_TLE_NO_LDS", "RRRMC_TLE_LDS")
    for label, Xt, Xl in models:
        for R in ([int(a) for a in sys.argv[2:]] or [8, 128, 2048]):
            out = {"model": label, "gamma": gamma, "lambda": lam, "beta_graph": beta_g, "beta": beta, "replicas": R, "iters": iters,
                   "classes": 2 * len(Xt.tables()), "max_deg": Xt.max_deg}
            legs = (("tle_rrr_lds", Xt, "rrr", {"RRRMC_TLE_LDS": "1"}), ("tle_rrr_global", Xt, "rrr", {"RRRMC_TLE_NO_LDS": "1"}),
                    ("le_rrr", Xl, "rrr", {}), ("tle_standard", Xt, "std", {}), ("le_standard", Xl, "std", {}))
            for name, X, sampler, env in legs:
                for k in envs:
                    os.environ.pop(k, None)
                os.environ.update(env)
                with pkg.Engine(X, R) as eng:
                    eng.seed(5)
                    eng.init_spins_random()
                    best = None
                    for rep in range(3):
                        acc = (eng.rrr_mc(beta, iters, iters) if sampler == "rrr" else eng.standard_mc(beta, iters, iters))[1]
                        _, sweep_ms, _ = eng.last_timing()
                        if rep and (best is None or sweep_ms < best[0]):
                            best = (sweep_ms, float(acc.mean()) / iters)
                    out[name] = {"kernel_iterations_per_s": float(R) * iters / (best[0] * 1e-3), "kernel_ms": best[0], "acceptance": best[1]}
                    if name.startswith("tle_rrr"):
                        out[name]["build"] = eng.tle_build()
            for k in envs:
                os.environ.pop(k, None)
            print(json.dumps(out), flush=True)


def bench_perc(Nk=1001, P=400, M=5, gamma=2.0, beta=0.4, iters=1 << 14, step=1 << 12, seed=0x5EED, reps=3):
    """GraphPercStepRE(1001, 400, 5), GraphPercStepLE(1001, 400, 5) (γ = 2, β = 0.4: bench_re's point over perceptron slices) and the
    stand-alone GraphPercStep(1001, 400): rrrMC through the thread and the LDS build and standardMC, kernel iterations/s per replica count
    (python tools/bench_models.py perc 128 1024 4096).  Every figure: one warm-up call, then `reps` timed calls, each continuing from the
    configuration the last one left; the median and the (min, max) of the kernel rate."""
    pkg = entry.load_package()
    X1 = pkg.GraphPercStep(Nk, P, seed=seed)
    envs = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS", "RRRMC_LE_NO_LDS", "RRRMC_LE_LDS")
    for R in ([int(a) for a in sys.argv[2:]] or [128, 1024, 4096]):
        it = max(step, iters * 1024 // max(R, 1024))
        for model, X, pre in (("GraphPercStepRE", pkg.GraphPercStepRE(X1, M, gamma, beta), "RRRMC_RE"),
                              ("GraphPercStepLE", pkg.GraphPercStepLE(X1, M, gamma, beta), "RRRMC_LE"), ("GraphPercStep", X1, None)):
            out = {"model": model, "Nk": Nk, "P": P, "M": M if pre else 1, "gamma": gamma, "beta": beta, "replicas": R, "iters": it}
            legs = (("rrr_thread", {pre + "_NO_LDS": "1"}), ("rrr_lds", {pre + "_LDS": "1"}), ("standard", {})) if pre else (("standard", {}),)
            for name, env in legs:
                for k in envs:
                    os.environ.pop(k, None)
                os.environ.update(env)
                eng = pkg.Engine(X, R)
                eng.seed(seed)
                eng.init_spins_random()
                rates = []
                for rep in range(reps + 1):                       # the first call is the warm-up
                    if name == "standard":
                        Es, acc = eng.standard_mc(beta, it, step)
                        staged = np.zeros(R)
                    else:
                        Es, acc, staged = eng.rrr_mc(beta, it, step)
                    _, sweep_ms, _ = eng.last_timing()
                    if rep:
                        rates.append(float(R) * it / (sweep_ms * 1e-3))
                out[name] = {"kernel_iterations_per_s": float(np.median(rates)), "min": min(rates), "max": max(rates),
                             "acceptance": float(acc.mean()) / it, "staged_frac": float(staged.mean()) / it,
                             "energy_per_spin": float(Es[:, -1].mean()) / X.N}
                eng.close()
            for k in envs:
                os.environ.pop(k, None)
            print(json.dumps(out), flush=True)


def bench_comm(P=400, M=5, gamma=2.0, beta=0.4, iters=1 << 14, step=1 << 12, seed=0x5EED, reps=3):
    """GraphCommStepRE / GraphCommStepLE(201, 5, 400, 5), GraphCommReLURE / GraphCommReLULE(168, 6, 400, 5) (γ = 2, β = 0.4: bench_perc's
    point over committee machine slices) and the stand-alone GraphCommStep(201, 5, 400), GraphCommReLU(168, 6, 400): rrrMC through the
    thread and the LDS build and standardMC, kernel iterations/s per replica count (python tools/bench_models.py comm 128 1024 4096), measured
    as bench_perc measures."""
    pkg = entry.load_package()
    envs = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS", "RRRMC_LE_NO_LDS", "RRRMC_LE_LDS")
    step_g, relu_g = pkg.GraphCommStep(201, 5, P, seed=seed), pkg.GraphCommReLU(168, 6, P, seed=seed)
    for R in ([int(a) for a in sys.argv[2:]] or [128, 1024, 4096]):
        it = max(step, iters * 1024 // max(R, 1024))
        for model, X, X1, pre in (("GraphCommStepRE", pkg.GraphCommStepRE(step_g, M, gamma, beta), step_g, "RRRMC_RE"),
                                  ("GraphCommStepLE", pkg.GraphCommStepLE(step_g, M, gamma, beta), step_g, "RRRMC_LE"),
                                  ("GraphCommStep", step_g, step_g, None),
                                  ("GraphCommReLURE", pkg.GraphCommReLURE(relu_g, M, gamma, beta), relu_g, "RRRMC_RE"),
                                  ("GraphCommReLULE", pkg.GraphCommReLULE(relu_g, M, gamma, beta), relu_g, "RRRMC_LE"),
                                  ("GraphCommReLU", relu_g, relu_g, None)):
            out = {"model": model, "K1": X1.K1, "K2": X1.K2, "P": P, "M": M if pre else 1, "gamma": gamma, "beta": beta, "replicas": R,
                   "iters": it}
            legs = (("rrr_thread", {pre + "_NO_LDS": "1"}), ("rrr_lds", {pre + "_LDS": "1"}), ("standard", {})) if pre else (("standard", {}),)
            for name, env in legs:
                for k in envs:
                    os.environ.pop(k, None)
                os.environ.update(env)
                eng = pkg.Engine(X, R)
                eng.seed(seed)
                eng.init_spins_random()
                rates = []
                for rep in range(reps + 1):                       # the first call is the warm-up
                    if name == "standard":
                        Es, acc = eng.standard_mc(beta, it, step)
                        staged = np.zeros(R)
                    else:
                        Es, acc, staged = eng.rrr_mc(beta, it, step)
                    _, sweep_ms, _ = eng.last_timing()
                    if rep:
                        rates.append(float(R) * it / (sweep_ms * 1e-3))
                out[name] = {"kernel_iterations_per_s": float(np.median(rates)), "min": min(rates), "max": max(rates),
                             "acceptance": float(acc.mean()) / it, "staged_frac": float(staged.mean()) / it,
                             "energy_per_spin": float(Es[:, -1].mean()) / X.N}
                eng.close()
            for k in envs:
                os.environ.pop(k, None)
            print(json.dumps(out), flush=True)


def _timed_legs(pkg, X, R, legs, envs, beta, it, step, seed, reps):
    """one warm-up call and `reps` timed calls per leg (name, env, sampler), each continuing from the configuration the last one left: the
    median and the (min, max) of the sampler kernel's rate (HIP events around the kernel), the acceptance of the last call"""
    out = {}
    for name, env, rrr in legs:
        for k in envs:
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = pkg.Engine(X, R)
        eng.seed(seed)
        eng.init_spins_random()
        rates, call_rates = [], []
        for rep in range(reps + 1):
            res = eng.rrr_mc(beta, it, step) if rrr else eng.standard_mc(beta, it, step)
            total_ms, sweep_ms, _ = eng.last_timing()
            if rep:
                rates.append(float(R) * it / (sweep_ms * 1e-3))
                call_rates.append(float(R) * it / (total_ms * 1e-3))
        # call_iterations_per_s: the events around the WHOLE call on the device — the energy / cache set-up of a fresh call and the layout
        # copies around the sampler kernel (the ensembles' slice-major copies, the SAT thread build's two transposes) included
        out[name] = {"kernel_iterations_per_s": float(np.median(rates)), "min": min(rates), "max": max(rates),
                     "call_iterations_per_s": float(np.median(call_rates)),
                     "acceptance": float(res[1].mean()) / it, "energy_per_spin": float(res[0][:, -1].mean()) / X.N}
        if not rrr and hasattr(X, "max_conn"):
            out[name]["build"] = eng.sat_build()
        if not rrr and type(X).__name__ == "GraphPSpin3":
            out[name]["build"] = eng.pspin_build()
        if not rrr and type(X).__name__ == "GraphPercXEntr":
            out[name]["build"] = eng.xentr_build()
        if type(X).__name__ == "GraphMixed" or type(getattr(X, "X1", None)).__name__ == "GraphMixed":
            out[name]["build"] = eng.af_build() if rrr else eng.mixed_build()
        eng.close()
    for k in envs:
        os.environ.pop(k, None)
    return out


def bench_sat(N=1000, K=3, alpha=4.2, beta=2.0, iters=1 << 16, step=1 << 12, seed=0x5EED, reps=3):
    """GraphSAT(1000, 3, 4.2) under standardMC at β = 2 through both builds (one wavefront per replica, one thread per replica), kernel
    iterations/s per replica count: python tools/bench_models.py sat 8 256 2048 8192"""
    pkg = entry.load_package()
    X = pkg.GraphSAT(N, K, alpha, seed=seed)
    envs = ("RRRMC_SAT_NO_WAVE", "RRRMC_SAT_WAVE")
    for R in ([int(a) for a in sys.argv[2:]] or [8, 256, 2048, 8192]):
        it = max(step, iters * 2048 // max(R, 2048))
        out = {"model": "GraphSAT", "N": N, "K": K, "alpha": alpha, "clauses": X.M, "max_conn": X.max_conn, "beta": beta, "replicas": R, "iters": it}
        out.update(_timed_legs(pkg, X, R, (("wave", {"RRRMC_SAT_WAVE": "1"}, False), ("thread", {"RRRMC_SAT_NO_WAVE": "1"}, False)), envs,
                               beta, it, step, seed, reps))
        print(json.dumps(out), flush=True)


def bench_satre(Nk=1001, K=3, alpha=4.2, P=400, M=5, gamma=2.0, beta=0.4, iters=1 << 14, step=1 << 12, seed=0x5EED, reps=3):
    """GraphSATRE(1001, 3, 4.2, 5) beside GraphPercStepRE(1001, 400, 5) (γ = 2, β = 0.4: bench_perc's point) under rrrMC through the thread and
    the LDS build, kernel iterations/s per chain count: python tools/bench_models.py satre 8 4096"""
    pkg = entry.load_package()
    envs = ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS")
    legs = (("rrr_thread", {"RRRMC_RE_NO_LDS": "1"}, True), ("rrr_lds", {"RRRMC_RE_LDS": "1"}, True), ("rrr_default", {}, True))
    for R in ([int(a) for a in sys.argv[2:]] or [8, 4096]):
        it = max(step, iters * 1024 // max(R, 1024))
        for model, X in (("GraphSATRE", pkg.GraphSATRE(Nk, K, alpha, M, gamma, beta, seed=seed)),
                         ("GraphPercStepRE", pkg.GraphPercStepRE(Nk, P, M, gamma, beta, seed=seed))):
            out = {"model": model, "Nk": Nk, "M": M, "gamma": gamma, "beta": beta, "replicas": R, "iters": it}
            out.update(_timed_legs(pkg, X, R, legs, envs, beta, it, step, seed, reps))
            print(json.dumps(out), flush=True)


def bench_xentr(N=1001, P=400, lam=1.0, beta=1.0, iters=1 << 14, step=1 << 8, seed=0x5EED, reps=3):
    """GraphPercXEntr(1001, 400, λ = 1) under standardMC at β = 1 through both builds (one wavefront per chain, one thread per chain), each with
    the loss table in LDS and in global memory, and the build the library picks by itself; GraphPercLinear(1001, 400) under the same call beside
    it for scale.  Kernel iterations/s per chain count: python tools/bench_models.py xentr 8 512 4096 32768"""
    pkg = entry.load_package()
    X = pkg.GraphPercXEntr(N, P, lam, seed=seed)
    XL = pkg.GraphPercLinear(N, P, seed=seed)
    envs = ("RRRMC_XENTR_NO_WAVE", "RRRMC_XENTR_WAVE", "RRRMC_XENTR_NO_LDS")
    legs = (("wave", {"RRRMC_XENTR_WAVE": "1"}, False), ("thread", {"RRRMC_XENTR_NO_WAVE": "1"}, False),
            ("wave_global_table", {"RRRMC_XENTR_WAVE": "1", "RRRMC_XENTR_NO_LDS": "1"}, False),
            ("thread_global_table", {"RRRMC_XENTR_NO_WAVE": "1", "RRRMC_XENTR_NO_LDS": "1"}, False), ("default", {}, False))
    for R in ([int(a) for a in sys.argv[2:]] or [8, 512, 4096, 32768]):
        it = max(step, iters * 1024 // max(R, 1024))
        out = {"model": "GraphPercXEntr", "N": N, "P": P, "lambda": lam, "beta": beta, "replicas": R, "iters": it}
        out.update(_timed_legs(pkg, X, R, legs, envs, beta, it, step, seed, reps))
        print(json.dumps(out), flush=True)
        out = {"model": "GraphPercLinear", "N": N, "P": P, "beta": beta, "replicas": R, "iters": it}
        out.update(_timed_legs(pkg, XL, R, (("standard", {}, False),), envs, beta, it, step, seed, reps))
        print(json.dumps(out), flush=True)


def bench_eare(L=10, D=3, M=5, gamma=1.5, lam=0.2, betas=(0.8, 0.2), iters=1 << 14, step=1 << 12, seed=0x5EED, reps=3):
    """GraphEARE(10, 3, 5) and GraphEATLE(10, 3, 5) (Nk = 1000, K = 6; γ = 1.5, λ = 0.2, graph β = sampler β = 0.8 and 0.2) under rrrMC through
    the global and the LDS build and under standardMC, beside GraphSKRE(1024, 5) at bench_re's point (γ = 2, β = 0.4) from the same build in
    the same job: kernel iterations/s per chain count (python tools/bench_models.py eare 8 512 4096; profiles/r18/sparse_ens.md)."""
    pkg = entry.load_package()
    models = [("GraphSKRE", pkg.GraphSKRE(1024, M, 2.0, 0.4, seed=seed), ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS"), 0.4)]
    for beta in betas:
        models.append(("GraphEARE", pkg.GraphEARE(L, D, M, gamma, beta, seed=seed), ("RRRMC_RE_NO_LDS", "RRRMC_RE_LDS"), beta))
        models.append(("GraphEATLE", pkg.GraphEATLE(L, D, M, gamma, lam, beta, seed=seed), ("RRRMC_TLE_NO_LDS", "RRRMC_TLE_LDS"), beta))
    for R in ([int(a) for a in sys.argv[2:]] or [8, 512, 4096]):
        it = max(step, iters * 1024 // max(R, 1024))
        for model, X, envs, b in models:
            legs = (("rrr_global", {envs[0]: "1"}, True), ("rrr_lds", {envs[1]: "1"}, True), ("rrr_default", {}, True), ("standard", {}, False))
            out = {"model": model, "Nk": X.Nk, "M": M, "beta": b, "replicas": R, "iters": it}
            out.update(_timed_legs(pkg, X, R, legs, envs, b, it, step, seed, reps))
            print(json.dumps(out), flush=True)


def bench_mixed(N=1001, P=400, K=3, alpha=4.2, beta=1.0, iters=1 << 14, step=1 << 8, seed=0x5EED, reps=3):
    """GraphMixed(GraphSK(1001), GraphPercStep(1001, 400), GraphSAT(1001, 3, 4.2)) under standardMC at β = 1 through both builds (one wavefront
    per chain, one thread per chain) and the build the library picks by itself, and rrrMC on GraphAddSubFields(h, mixed) with Gaussian fields
    through its two builds.  Kernel iterations/s per chain count: python tools/bench_models.py mixed 8 512 4096 16384"""
    pkg = entry.load_package()
    X = pkg.GraphMixed(pkg.GraphSK(N, seed=seed), pkg.GraphPercStep(N, P, seed=seed), pkg.GraphSAT(N, K, alpha, seed=seed))
    Xw = pkg.GraphAddSubFields(np.random.default_rng(seed).normal(size=N), X)
    envs = ("RRRMC_MIXED_NO_WAVE", "RRRMC_MIXED_WAVE", "RRRMC_AF_NO_LDS")
    legs = (("wave", {"RRRMC_MIXED_WAVE": "1"}, False), ("thread", {"RRRMC_MIXED_NO_WAVE": "1"}, False), ("default", {}, False))
    rlegs = (("rrr_lds", {}, True), ("rrr_global", {"RRRMC_AF_NO_LDS": "1"}, True))
    for R in ([int(a) for a in sys.argv[2:]] or [8, 512, 4096, 16384]):
        it = max(step, iters * 1024 // max(R, 1024))
        out = {"model": "GraphMixed(SK, PercStep, SAT)", "N": N, "P": P, "clauses": X.graphs[2].M, "beta": beta, "replicas": R, "iters": it}
        out.update(_timed_legs(pkg, X, R, legs, envs, beta, it, step, seed, reps))
        print(json.dumps(out), flush=True)
        out = {"model": "GraphAddSubFields(h, GraphMixed(SK, PercStep, SAT))", "N": N, "beta": beta, "replicas": R, "iters": it}
        out.update(_timed_legs(pkg, Xw, R, rlegs, envs, beta, it, step, seed, reps))
        print(json.dumps(out), flush=True)


def bench_pspin3(N=3000, Ks=(3, 8), alpha=4.2, beta=1.0, iters=1 << 16, step=1 << 12, seed=0x5EED, reps=3):
    """GraphPSpin3(3000, 3) and GraphPSpin3(3000, 8) under standardMC at β = 1 through both builds (one wavefront per chain with 64 iterations
    side by side, one thread per chain) and the build the library picks by itself, and GraphSAT(3000, 3, 4.2) through its two builds under the
    same call as the yardstick.  Kernel iterations/s per chain count (profiles/r20/pspin3.md):
    python tools/bench_models.py pspin3 8 32 128 512 2048 8192 16384 32768 65536"""
    pkg = entry.load_package()
    envs = ("RRRMC_PSPIN_NO_WAVE", "RRRMC_PSPIN_WAVE", "RRRMC_SAT_NO_WAVE", "RRRMC_SAT_WAVE")
    models = [("GraphPSpin3", {"N": N, "K": K}, pkg.GraphPSpin3(N, K, seed=seed),
               (("wave", {"RRRMC_PSPIN_WAVE": "1"}, False), ("thread", {"RRRMC_PSPIN_NO_WAVE": "1"}, False), ("default", {}, False))) for K in Ks]
    models.append(("GraphSAT", {"N": N, "K": 3, "alpha": alpha}, pkg.GraphSAT(N, 3, alpha, seed=seed),
                   (("wave", {"RRRMC_SAT_WAVE": "1"}, False), ("thread", {"RRRMC_SAT_NO_WAVE": "1"}, False))))
    for R in ([int(a) for a in sys.argv[2:]] or [8, 32, 128, 512, 2048, 8192, 16384, 32768, 65536]):
        it = max(step, iters * 2048 // max(R, 2048))
        for model, par, X, legs in models:
            out = {"model": model, **par, "beta": beta, "replicas": R, "iters": it}
            out.update(_timed_legs(pkg, X, R, legs, envs, beta, it, step, seed, reps))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "sk"
    {"pspin3": bench_pspin3, "mixed": bench_mixed, "eare": bench_eare, "sk": bench_sk, "ea": bench_ea, "quant": bench_quant, "spf": bench_spf, "spf_fast": bench_spf_fast, "dbl": bench_dbl, "ea_random": bench_ea_random, "re": bench_re, "le": bench_le, "perc": bench_perc, "comm": bench_comm, "sat": bench_sat, "satre": bench_satre, "tle": bench_tle, "xentr": bench_xentr}[which]()
