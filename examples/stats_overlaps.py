#!/usr/bin/env python3
"""The reference's equilibration test `stats_overlaps` (scripts/scripts.jl:459-522) on the MI355X engine: the two-time self overlap
<q^2>(t) of one run (`parseovs`) printed beside the cross overlap <x^2>(t) of two independent runs (`parsexovs`).  When the two
agree the run has equilibrated on that time scale.  Here the "two runs" are two replicas of one batch on the same GraphRRG(N, 3)
instance, and every overlap is computed on the device from the snapshots the hook kept in HBM.  The last snapshot also gives the
order-parameter distribution P(q) over all replica pairs: <q^2>, <q^4> and the Binder ratio (`overlap_hist` -> `overlap_moments`).

  python examples/stats_overlaps.py [--N 512] [--beta 1.5] [--samples 24] [--step 2000] [--replicas 16] [--pairs 3]

Differences from the script: the clock is the Monte Carlo time of the samples (the reference reads wall-clock times from its log
files), so the table is the same on every machine; the default sizes are small and the run takes seconds.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--beta", type=float, default=1.5)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--step", type=int, default=2000)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=3, help="replica pairs (0, 1), (2, 3), ... used as the two runs of parsexovs")
    ap.add_argument("--seedx", type=int, default=8370000274)  # graph seed, scripts.jl:460
    ap.add_argument("--seed", type=int, default=6540000789)   # sampler seed
    ap.add_argument("--incr", type=float, default=2.0)        # scripts.jl:462
    args = ap.parse_args(argv)

    pkg = entry.load_package()
    X = pkg.GraphRRG(args.N, args.K, seed=args.seedx)
    R = args.replicas
    npairs = max(1, min(args.pairs, R // 2))
    with pkg.Engine(X, R) as eng:
        eng.seed(args.seed)
        eng.init_spins_random()
        log = pkg.SnapshotLog(eng, args.samples)
        pkg.standardMC(X, args.beta, args.step * args.samples, step=args.step, seed=args.seed, hook=log, engine=eng, quiet=True)
        ts = [float(t) for t in log.mctimes]                  # the clock of every run: Monte Carlo time
        lr = list(pkg.log_range(ts[0], ts[-1], st0=ts[0], incr=args.incr))
        mq2, sq2 = pkg.parseovs(eng, ts, lr)                  # [windows, R]: the self overlap of every replica
        cross = [pkg.parsexovs(eng, ts, ts, lr, 2 * k, 2 * k + 1) for k in range(npairs)]
        hist = eng.overlap_hist(log.count - 1, log.count - 1)
        mom = pkg.overlap_moments(hist, X.N)
    rows = []
    print("#time self std cross std")                          # scripts.jl:508
    for w in range(min(len(mq2), min(len(c[0]) for c in cross))):
        runs = [r for k in range(npairs) for r in (2 * k, 2 * k + 1)]
        # (mq2s1 + mq2s2) / 2 of the script, averaged over the pairs
        s_m, s_s = float(np.mean(mq2[w, runs])), float(np.mean(sq2[w, runs]))
        x_m, x_s = float(np.mean([c[0][w] for c in cross])), float(np.mean([c[1][w] for c in cross]))
        if any(np.isnan(v) for v in (s_m, s_s, x_m, x_s)):     # the script warns and skips such a window (:514)
            continue
        rows.append((lr[w], s_m, s_s, x_m, x_s))
        print("%g %.6f %.6f %.6f %.6f" % rows[-1])
    print("P(q) of the last snapshot over %d replica pairs: <q^2> = %.6f  <q^4> = %.6f  <|q|> = %.6f  Binder = %.4f"
          % (mom["pairs"], mom["q2"], mom["q4"], mom["absq"], mom["binder"]))
    return rows, mom


if __name__ == "__main__":
    main()
