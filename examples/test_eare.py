#!/usr/bin/env python3
"""A Robust Ensemble run on an Edwards-Anderson lattice, after examples/test_reising.py (the reference's `scripts/scripts.jl:test_REIsing`,
:866-963, with GraphEARE in the place of GraphSKRE): Metropolis and RRR on one GraphEARE(L, D, M, γ, β) instance (M replicas of one lattice
with couplings uniform in [-2, 2), coupled by GraphRE), logging `#mctime acc meanRE clocktime E` with meanRE = mean(REenergies(X)) read from
the device inside the hook at every sample.

  python examples/test_eare.py [--L 10] [--D 3] [--M 5] [--beta 0.8] [--gamma 1.5] [--step 10000] [--t-limit 60]

A run ends through its hook once `t_limit` seconds have passed, or after `--samples` samples.  Randomness comes from the engine's Philox
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
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--D", type=int, default=3)
    ap.add_argument("--M", type=int, default=5)
    ap.add_argument("--beta", type=float, default=0.8)
    ap.add_argument("--gamma", type=float, default=1.5)
    ap.add_argument("--samples", type=int, default=10 ** 10)       # iters = samples * step
    ap.add_argument("--step", type=int, default=10_000)
    ap.add_argument("--seedx", type=int, default=8370000274)
    ap.add_argument("--seed", type=int, default=6540000789)
    ap.add_argument("--met-factor", type=float, default=20.8)      # Metropolis iterations per RRR iteration (scripts.jl:877)
    ap.add_argument("--t-limit", type=float, default=60.0)
    ap.add_argument("--algs", default="met,rrr")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    pkg = entry.load_package()
    out = args.out or "output_EARE_L%d_D%d_M%d_beta%s_gamma%s_tmax%s_step%d" % (args.L, args.D, args.M, args.beta, args.gamma, args.t_limit, args.step)
    os.makedirs(out, exist_ok=True)
    X = pkg.GraphEARE(args.L, args.D, args.M, args.gamma, args.beta, seed=args.seedx)
    for alg in args.algs.split(","):
        assert alg in ("met", "rrr")
        rstep = round(args.step * (args.met_factor if alg == "met" else 1.0))
        fn = os.path.join(out, "output_%s_sx%d_s%d.txt" % (alg, args.seedx, args.seed))
        with open(fn, "w") as f:
            print("#mctime acc meanRE clocktime E", file=f)
            t0 = time.time()

            def hook(mct, X_, C, acc, E):
                t = time.time() - t0
                meanRE = float(np.mean(pkg.REenergies(X_)))
                print("%d %d %r %r %r" % (mct, int(np.asarray(acc).reshape(-1)[0]), meanRE, t, float(np.asarray(E).reshape(-1)[0])), file=f)
                f.flush()
                return t < args.t_limit

            sampler = pkg.standardMC if alg == "met" else pkg.rrrMC
            sampler(X, args.beta, rstep * args.samples, step=rstep, seed=args.seed, hook=hook, quiet=True)
        print(fn)
    return 0


if __name__ == "__main__":
    sys.exit(main())
