#!/usr/bin/env python3
"""A mixed model, after the second example of the reference's `GraphMixed` docstring (src/graphs/Mixed.jl:10-13):

    X = GraphMixed(GraphSK(31), GraphPercStep(31, 30), GraphSAT(31, 3, 4.2))

— a spin glass with a learning term and a K-SAT constraint on one set of 31 spins — under Metropolis (`standardMC` on the mix) and under
RRR (`rrrMC` on `GraphAddSubFields(h, X)`: the fields only shape the proposals, the stationary law is the mix's own), in the style of
examples/test_eare.py.  The log is `#mctime acc E_SK E_Perc E_SAT clocktime E`, the three components' energies read from the device inside the
hook at every sample (`mixed_energies`).

  python examples/test_mixed.py [--N 31] [--P 30] [--alpha 4.2] [--beta 1.0] [--step 1000] [--samples 20] [--t-limit 60]

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
    ap.add_argument("--N", type=int, default=31)
    ap.add_argument("--P", type=int, default=30)
    ap.add_argument("--alpha", type=float, default=4.2)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--field", type=float, default=0.5)            # scale of the Gaussian proposal fields of the RRR run
    ap.add_argument("--samples", type=int, default=20)             # iters = samples * step
    ap.add_argument("--step", type=int, default=1000)
    ap.add_argument("--seedx", type=int, default=8370000274)
    ap.add_argument("--seed", type=int, default=6540000789)
    ap.add_argument("--t-limit", type=float, default=60.0)
    ap.add_argument("--algs", default="met,rrr")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    pkg = entry.load_package()
    out = args.out or "output_Mixed_N%d_P%d_alpha%s_beta%s_tmax%s_step%d" % (args.N, args.P, args.alpha, args.beta, args.t_limit, args.step)
    os.makedirs(out, exist_ok=True)
    X = pkg.GraphMixed(pkg.GraphSK(args.N, seed=args.seedx), pkg.GraphPercStep(args.N, args.P, seed=args.seedx), pkg.GraphSAT(args.N, 3, args.alpha, seed=args.seedx))
    h = args.field * np.random.default_rng(args.seedx).normal(size=args.N)
    for alg in args.algs.split(","):
        assert alg in ("met", "rrr")
        G = X if alg == "met" else pkg.GraphAddSubFields(h, X)
        fn = os.path.join(out, "output_%s_sx%d_s%d.txt" % (alg, args.seedx, args.seed))
        with open(fn, "w") as f:
            print("#mctime acc E_SK E_Perc E_SAT clocktime E", file=f)
            t0 = time.time()

            def hook(mct, X_, C, acc, E):
                t = time.time() - t0
                parts = np.asarray(pkg.mixed_energies(X_)).reshape(-1)
                print("%d %d %r %d %d %r %r" % (mct, int(np.asarray(acc).reshape(-1)[0]), float(parts[0]), int(parts[1]), int(parts[2]), t,
                                                float(np.asarray(E).reshape(-1)[0])), file=f)
                f.flush()
                return t < args.t_limit

            sampler = pkg.standardMC if alg == "met" else pkg.rrrMC
            sampler(G, args.beta, args.step * args.samples, step=args.step, seed=args.seed, hook=hook, quiet=True)
        print(fn)
    return 0


if __name__ == "__main__":
    sys.exit(main())
