#!/usr/bin/env python3
"""Parallel tempering on a three-dimensional Edwards-Anderson glass with Gaussian couplings, GraphEANormal(L, 3), on the MI355X engine:
a ladder of inverse temperatures (one device context each), R independent ladders side by side, exchange attempts between neighbouring
temperatures every `--iters` single-spin attempts.  Printed per temperature: the exchange acceptance with the next temperature, the mean
energy per spin, and <q^2> and the Binder ratio of the overlap distribution P(q) over the R replicas of that temperature.  Beside it:
the same figures from independent runs of equal length at the coldest beta alone (no exchanges), as examples/stats_overlaps.py prints the
self overlap beside the cross overlap.  The program prints both and claims nothing about either.

  python examples/pt_ea.py [--L 6] [--betas 0.5,0.56,0.62,0.69,0.77,0.86,0.96,1.07,1.19,1.32] [--replicas 64] [--rounds 200] [--iters 216]
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
    ap.add_argument("--L", type=int, default=6)
    ap.add_argument("--D", type=int, default=3)
    ap.add_argument("--betas", type=str, default="0.5,0.56,0.62,0.69,0.77,0.86,0.96,1.07,1.19,1.32")
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--iters", type=int, default=0, help="single-spin attempts between two exchange rounds (default: one sweep, N)")
    ap.add_argument("--seedx", type=int, default=8370000274)  # graph seed
    ap.add_argument("--seed", type=int, default=6540000789)   # ladder seed
    args = ap.parse_args(argv)

    pkg = entry.load_package()
    X = pkg.GraphEANormal(args.L, args.D, seed=args.seedx)
    betas = [float(b) for b in args.betas.split(",")]
    R, N = args.replicas, X.N
    iters = args.iters if args.iters > 0 else N
    with pkg.ParallelTempering(X, betas, R=R, seed=args.seed) as pt:
        t0 = time.perf_counter()
        pt.run(args.rounds, iters)
        wall = time.perf_counter() - t0
        E = np.stack(pt.energies)                             # [rounds][T][R]
        half = E[len(E) // 2:]                                # the second half of the run
        rows = []
        print("#beta accept_next <E>/N <q^2> Binder")
        for t, beta in enumerate(pt.betas):
            mom = pkg.overlap_moments(pt.overlap_hist(t), N)
            acc = float(pt.accept_rate[t]) if t + 1 < pt.T else float("nan")
            rows.append((float(beta), acc, float(half[:, t].mean()) / N, mom["q2"], mom["binder"]))
            print("%g %.4f %.6f %.6f %.4f" % rows[-1])
        print("(accept_next: the fraction of exchanges accepted with the next beta of the ladder; nan in the last row, which has none)")
        trips = int(pt.round_trips.sum())
        print("round trips: %d over %d ladders; %d rounds of %d attempts in %.2f s = %.3e attempts/s"
              % (trips, R, pt.round, iters, wall, pt.T * R * pt.round * iters / wall))
    # the coldest temperature alone: the same number of attempts, no exchanges
    cold = max(betas)
    with pkg.Engine(X, R) as eng:
        eng.seed(pkg.ladder_seed(args.seed, len(betas)))      # a seed no context of the ladder had
        eng.init_spins_random()
        for _ in range(args.rounds):
            eng.standard_mc(cold, iters, iters, want_energies=False)
        mom = pkg.overlap_moments(eng.overlap_hist(-1, -1), N)
        alone = (cold, float(eng.energy().mean()) / N, mom["q2"], mom["binder"])
    print("alone at beta %g: <E>/N %.6f  <q^2> %.6f  Binder %.4f" % alone)
    return rows, trips, alone


if __name__ == "__main__":
    main()
