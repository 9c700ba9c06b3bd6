#!/usr/bin/env python3
"""The reference's Robust Ensemble experiment `scripts/scripts.jl:test_REIsing` (:866-963) on the MI355X engine: Metropolis and RRR on one
GraphSKRE(N, M, γ, β) instance (M replicas of one binary SK disorder coupled by GraphRE), logging `#mctime acc meanRE clocktime E` with
meanRE = mean(REenergies(X)) read from the device inside the hook at every sample.

  python examples/test_reising.py [--N 1024] [--M 5] [--beta 0.4] [--gamma 2.0] [--step 10000] [--t-limit 250] [--ntests 1]

As in the script the Metropolis leg does `met_factor` (20.8) iterations per RRR iteration, and a run ends through its hook once `t_limit`
seconds have passed (the script's `iters = 10^14` is only a bound; `--samples` sets it here).  Randomness comes from the engine's Philox
streams; the sampled configurations are not saved.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)                 # scripts.jl:866-870
    ap.add_argument("--M", type=int, default=5)
    ap.add_argument("--beta", type=float, default=0.4)
    ap.add_argument("--gamma", type=float, default=2.0)
    ap.add_argument("--samples", type=int, default=10 ** 10)       # iters = samples * step (the script: 10^14 / step)
    ap.add_argument("--step", type=int, default=10_000)
    ap.add_argument("--seedx", type=int, default=8370000274)
    ap.add_argument("--seed", type=int, default=6540000789)
    ap.add_argument("--seedst", type=int, default=10_000)
    ap.add_argument("--ntests", type=int, default=1)
    ap.add_argument("--met-factor", type=float, default=20.8)      # scripts.jl:877
    ap.add_argument("--rrr-factor", type=float, default=1.0)
    ap.add_argument("--t-limit", type=float, default=250.0)        # scripts.jl:879
    ap.add_argument("--algs", default="met,rrr")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    pkg = entry.load_package()
    out = args.out or "output_REIsing_N%d_M%d_beta%s_gamma%s_tmax%s_step%d" % (args.N, args.M, args.beta, args.gamma, args.t_limit, args.step)
    os.makedirs(out, exist_ok=True)
    seed, seedx = args.seed, args.seedx
    for _ in range(args.ntests):
        X = pkg.GraphSKRE(args.N, args.M, args.gamma, args.beta, seed=seedx)
        for alg in args.algs.split(","):
            assert alg in ("met", "rrr")                           # scripts.jl:884
            rstep = round(args.step * (args.met_factor if alg == "met" else args.rrr_factor))
            riters = rstep * args.samples
            fn = os.path.join(out, "output_%s_sx%d_s%d.txt" % (alg, seedx, seed))
            with open(fn, "w") as f:
                print("#mctime acc meanRE clocktime E", file=f)
                t0 = time.time()

                def hook(mct, X_, C, acc, E):                      # scripts.jl:901-907
                    t = time.time() - t0
                    meanRE = float(np.mean(pkg.REenergies(X_)))
                    print("%d %d %r %r %r" % (mct, int(np.asarray(acc).reshape(-1)[0]), meanRE, t, float(np.asarray(E).reshape(-1)[0])), file=f)
                    f.flush()
                    return t < args.t_limit

                sampler = pkg.standardMC if alg == "met" else pkg.rrrMC
                sampler(X, args.beta, riters, step=rstep, seed=seed, hook=hook, quiet=True)
            print(fn)
        seed += args.seedst
        seedx += args.seedst
    return 0


if __name__ == "__main__":
    sys.exit(main())
