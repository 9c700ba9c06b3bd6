#!/usr/bin/env python3
"""A short anneal of the regular 3-spin model, `GraphPSpin3(N, K)` (src/graphs/PSpin3.jl): the textbook glassy system after RRG, EA and SK.

    X = GraphPSpin3(3000, 3)

Metropolis (`standardMC` on the graph) through a ladder of inverse temperatures, each rung continuing from the configuration the last one
left, and — with `--algs met,rrr` — the same ladder under RRR on `GraphAddSubFields(h, X)` (the fields only shape the proposals, the
stationary law is the graph's own), in the style of examples/test_mixed.py.  The log is `#beta mctime acc E E/N clocktime`: E/N falls and
freezes above its floor of −K/3 (every triple of every layer satisfied).

  python examples/test_pspin3.py [--N 3000] [--K 3] [--betas 0.2,0.5,1,1.5,2,3] [--step 3000] [--samples 10] [--t-limit 60]

A rung ends through its hook once `t_limit` seconds have passed since the start, or after `--samples` samples.  Randomness comes from the
engine's Philox streams; the sampled configurations are not saved.
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
    ap.add_argument("--N", type=int, default=3000)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--betas", default="0.2,0.5,1,1.5,2,3")
    ap.add_argument("--field", type=float, default=0.5)            # scale of the Gaussian proposal fields of the RRR run
    ap.add_argument("--samples", type=int, default=10)             # iterations per rung = samples * step
    ap.add_argument("--step", type=int, default=3000)
    ap.add_argument("--seedx", type=int, default=8370000274)
    ap.add_argument("--seed", type=int, default=6540000789)
    ap.add_argument("--t-limit", type=float, default=60.0)
    ap.add_argument("--algs", default="met")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    pkg = entry.load_package()
    out = args.out or "output_PSpin3_N%d_K%d_tmax%s_step%d" % (args.N, args.K, args.t_limit, args.step)
    os.makedirs(out, exist_ok=True)
    X = pkg.GraphPSpin3(args.N, args.K, seed=args.seedx)
    h = args.field * np.random.default_rng(args.seedx).normal(size=args.N)
    betas = [float(b) for b in args.betas.split(",")]
    for alg in args.algs.split(","):
        assert alg in ("met", "rrr")
        G = X if alg == "met" else pkg.GraphAddSubFields(h, X)
        sampler = pkg.standardMC if alg == "met" else pkg.rrrMC
        fn = os.path.join(out, "output_%s_sx%d_s%d.txt" % (alg, args.seedx, args.seed))
        with open(fn, "w") as f:
            print("#beta mctime acc E E/N clocktime", file=f)
            t0 = time.time()
            C = None
            for rung, beta in enumerate(betas):
                def hook(mct, X_, C_, acc, E):
                    t = time.time() - t0
                    e = float(np.asarray(E).reshape(-1)[0])
                    print("%r %d %d %r %r %r" % (beta, mct, int(np.asarray(acc).reshape(-1)[0]), e, e / args.N, t), file=f)
                    f.flush()
                    return t < args.t_limit

                # every rung is a call of its own from the configuration the last one left, on streams of its own (seed + rung)
                _, C = sampler(G, beta, args.step * args.samples, step=args.step, seed=args.seed + rung, hook=hook, C0=C, quiet=True)
        print(fn)
    return 0


if __name__ == "__main__":
    sys.exit(main())
