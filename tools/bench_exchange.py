"""What a replica exchange between two contexts costs (rrrmc_exchange_async), beside what it is measured against at the same
shape: one sweep of one context, a device-to-device copy of the bytes the swap moves, and the host route a user had before it (two
energy calls, get_spins, a numpy swap, set_spins).  Then the end-to-end rate of examples/pt_ea.py's ladder beside the sum of its
contexts' plain standardMC rates.

  python tools/bench_exchange.py [--out profiles/r22/exchange.md] [--repeats 5]

Without --shape the script starts one child process per shape, each under its own `timeout`, one after the other, and stops at the
first that fails; it never opens the device itself.  Each child prints one JSON line; the parent renders the lines into the Markdown
file, stamped with the sources they were measured on.

Timing.  The ABI has no event pair around an exchange, so device times are host clocks around a QUEUE of n identical asynchronous calls
closed by one synchronise, divided by n (n is chosen so that a sample lasts about a quarter of a second: the launch overhead of the
host is hidden behind the device's queue as long as the device is the slower side; where it is not, the figure is the host's enqueue
rate and an upper bound of the device time).  Medians of `--repeats` samples after a warm-up; min and max beside them."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {   # name -> (graph, N, R, time limit of the child in seconds)
    "rrg4096_r8192": ("GraphRRG", 4096, 8192, 300),
    "rrgnormal4096_r8192": ("GraphRRGNormal", 4096, 8192, 400),
    "sknormal1024_r2048": ("GraphSKNormal", 1024, 2048, 400),
    "pt_ea_l6": ("GraphEANormal", 216, 64, 300),
}
SOURCES = ["rrrmc.jl_amd/csrc/pt_kernels.hpp", "rrrmc.jl_amd/csrc/pt_core.hpp", "rrrmc.jl_amd/csrc/host_pt.hpp", "rrrmc.jl_amd/tempering.py"]
ANALYSIS_HEADING = "## What the figures say"            # written by hand below the tables of the Markdown file; render() keeps it
PT_BETAS = (0.5, 0.56, 0.62, 0.69, 0.77, 0.86, 0.96, 1.07, 1.19, 1.32)          # the default ladder of examples/pt_ea.py


def _queue_ms(enqueue, sync, repeats, n=None):
    """milliseconds per call of a queue of n calls closed by one sync: (median, min, max, n)"""
    enqueue(); sync()
    if n is None:
        t0 = time.perf_counter()
        for _ in range(8):
            enqueue()
        sync()
        n = max(8, min(2000, int(0.25 / max((time.perf_counter() - t0) / 8, 1e-7))))
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(n):
            enqueue()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3 / n)
    return statistics.median(ts), min(ts), max(ts), n


def _native_bytes(name, N, R):
    if name == "GraphRRG":
        return 4 * ((R + 31) // 32) * N
    if name in ("GraphRRGNormal", "GraphEANormal"):
        return 8 * ((R + 63) // 64) * N
    return ((R + 7) // 8) * N


def child(shape, repeats):
    import __graft_entry__ as entry
    pkg = entry.load_package()
    name, N, R, _ = SHAPES[shape]
    if shape == "pt_ea_l6":
        return child_pt(pkg, repeats)
    X = pkg.GraphRRG(N, 3, seed=7) if name == "GraphRRG" else pkg.GraphRRGNormal(N, 3, seed=7) if name == "GraphRRGNormal" else pkg.GraphSKNormal(N, seed=7)
    ba, bb = 1.0, 0.9
    out = {"shape": shape, "graph": "%s(%d%s)" % (name, N, "" if name == "GraphSKNormal" else ", 3"), "R": R, "native_bytes": _native_bytes(name, N, R)}
    with pkg.Engine(X, R) as a, pkg.Engine(X, R) as b:
        for e, s in ((a, 11), (b, 12)):
            e.seed(s)
            e.init_spins_random()
            e.standard_mc(1.0, 4 * N, 4 * N)
        both = lambda: (a.sync(), b.sync())
        rnd = [0]

        def xchg():
            rnd[0] += 1
            a.exchange(b, ba, bb, 5, rnd[0], wait=False)
        # back to back: every exchange but the first finds no live tracked energy, so each is the energy passes plus the launch
        out["exchange_recompute_ms"] = _queue_ms(xchg, both, repeats)
        sw = a.exchange(b, ba, bb, 5, 0)[0]
        out["accepted_fraction"] = float(sw.mean())
        # one sweep of one context, and a round of one sweep on both contexts with and without the exchange behind it
        out["sweep_ms"] = _queue_ms(lambda: a.standard_mc_async(ba, N, N), a.sync, repeats)

        def round_plain():
            a.standard_mc_async(ba, N, N)
            b.standard_mc_async(bb, N, N)

        def round_xchg():
            round_plain()
            xchg()
        n = out["sweep_ms"][3]
        out["round_two_sweeps_ms"] = _queue_ms(round_plain, both, repeats, n)
        out["round_two_sweeps_exchange_ms"] = _queue_ms(round_xchg, both, repeats, n)
        # the bytes the swap moves: both buffers in, both out = a device-to-device copy of two buffers
        g = C.c_double(0.0)
        pkg._lib.check(pkg.lib().rrrmc_device_copy_bandwidth(0, 2 * out["native_bytes"], 50, C.byref(g)))
        out["copy_gbps"] = g.value
        out["copy_ms"] = 2 * 2 * out["native_bytes"] / (g.value * 1e9) * 1e3 if g.value > 0 else None
        # the host route
        def host_route():
            Ea, Eb = np.asarray(a.energy(), np.float64), np.asarray(b.energy(), np.float64)
            ca, cb = a.get_config(), b.get_config()
            x = (ba - bb) * (Ea - Eb)
            s = (x >= 0) | (np.random.default_rng(1).random(R) < np.exp(np.minimum(x, 0.0)))
            sa, sb = np.where(s[:, None], cb.s, ca.s), np.where(s[:, None], ca.s, cb.s)
            a.set_config(pkg.Config(N, R, np.ascontiguousarray(sa)))
            b.set_config(pkg.Config(N, R, np.ascontiguousarray(sb)))
        host_route()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            host_route()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["host_route_ms"] = (statistics.median(ts), min(ts), max(ts), 1)
    print(json.dumps(out))


def child_pt(pkg, repeats):
    """examples/pt_ea.py's ladder: attempts per second of the whole driver beside the sum of its contexts' plain standardMC rates"""
    X = pkg.GraphEANormal(6, 3, seed=8370000274)
    R, N, rounds = 64, 216, 200
    out = {"shape": "pt_ea_l6", "graph": "GraphEANormal(6, 3)", "R": R, "T": len(PT_BETAS), "rounds": rounds, "iters": N}
    rates = []
    with pkg.ParallelTempering(X, PT_BETAS, R=R, seed=6540000789) as pt:
        pt.run(20, N)
        for _ in range(repeats):
            t0 = time.perf_counter()
            pt.run(rounds, N)
            rates.append(len(PT_BETAS) * R * rounds * N / (time.perf_counter() - t0))
        out["accept_rate"] = [float(x) for x in pt.accept_rate]
        out["pt_attempts_per_s"] = (statistics.median(rates), min(rates), max(rates))
        # the same contexts without exchanges: every round queued on all of them, one wait per round (what the driver's wait costs) ...
        plain, queued = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(rounds):
                for t in range(pt.T):
                    pt.engine(t).standard_mc_async(PT_BETAS[t], N, N)
                for t in range(pt.T):
                    pt.engine(t).sync()
            plain.append(len(PT_BETAS) * R * rounds * N / (time.perf_counter() - t0))
            # ... and with one wait at the very end (the device's own rate for these calls)
            t0 = time.perf_counter()
            for _ in range(rounds):
                for t in range(pt.T):
                    pt.engine(t).standard_mc_async(PT_BETAS[t], N, N)
            for t in range(pt.T):
                pt.engine(t).sync()
            queued.append(len(PT_BETAS) * R * rounds * N / (time.perf_counter() - t0))
        out["plain_sync_per_round_attempts_per_s"] = (statistics.median(plain), min(plain), max(plain))
        out["plain_queued_attempts_per_s"] = (statistics.median(queued), min(queued), max(queued))
    print(json.dumps(out))


def _fmt(v, unit="ms"):
    if v is None:
        return "—"
    med, lo, hi = v[0], v[1], v[2]
    if unit == "ms":
        return "%.4f (%.4f – %.4f)" % (med, lo, hi)
    return "%.3e (%.3e – %.3e)" % (med, lo, hi)


def render(rows, path, repeats):
    import bench
    L = ["# Replica exchange between contexts: what it costs", "",
         "Written by `tools/bench_exchange.py --repeats %d` on one MI355X; source stamp `%s` over %s." % (repeats, bench.source_stamp(SOURCES), ", ".join("`%s`" % s for s in SOURCES)),
         "Device times are host clocks around a queue of n identical asynchronous calls closed by one synchronise, divided by n",
         "(the ABI has no event pair around an exchange; per-kernel device times from a profiler run are further down); median (min – max) of the samples, milliseconds per call.", ""]
    L += ["| shape | R | native bytes per context | exchange, energies recomputed | one sweep (N attempts) of one context | two sweeps (both contexts) | two sweeps + exchange on the tracked energy | n | D2D copy of the swapped bytes | host route | accepted |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["shape"] == "pt_ea_l6":
            continue
        L.append("| `%s` | %d | %d | %s | %s | %s | %s | %d | %s ms at %.0f GB/s | %s | %.2f |" % (
            r["graph"], r["R"], r["native_bytes"], _fmt(r["exchange_recompute_ms"]), _fmt(r["sweep_ms"]), _fmt(r["round_two_sweeps_ms"]),
            _fmt(r["round_two_sweeps_exchange_ms"]), r["sweep_ms"][3], "%.4f" % r["copy_ms"] if r["copy_ms"] else "—", r["copy_gbps"], _fmt(r["host_route_ms"]), r["accepted_fraction"]))
    for r in rows:
        if r["shape"] != "pt_ea_l6":
            continue
        L += ["", "## The ladder of `examples/pt_ea.py`", "",
              "`%s`, %d temperatures × %d replicas, %d rounds of %d attempts (one sweep) per sample; attempts per second, median (min – max)." % (r["graph"], r["T"], r["R"], r["rounds"], r["iters"]), "",
              "| what | attempts/s |", "|---|---|",
              "| `ParallelTempering.run` (sampling, exchanges, one wait and the bookkeeping per round) | %s |" % _fmt(r["pt_attempts_per_s"], "rate"),
              "| the same standardMC calls on the same contexts, no exchange, one wait per round | %s |" % _fmt(r["plain_sync_per_round_attempts_per_s"], "rate"),
              "| the same calls queued, one wait at the end | %s |" % _fmt(r["plain_queued_attempts_per_s"], "rate"),
              "", "Exchange acceptance per pair: %s." % ", ".join("%.3f" % x for x in r["accept_rate"][:-1] + r["accept_rate"][-1:])]
    # the hand-written reading of the figures (from its heading to the raw block) survives a rerun: it is carried over from the file being replaced
    kept = []
    if os.path.exists(path):
        old = open(path).read()
        i, j = old.find(ANALYSIS_HEADING), old.find("<!-- raw -->")
        if 0 <= i < j:
            kept = [old[i:j].rstrip("\n")]
    L += [""] + kept + ["", "<!-- raw -->", "```json"] + [json.dumps(r) for r in rows] + ["```", ""]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "exchange.md"))
    args = ap.parse_args()
    if args.shape:
        child(args.shape, args.repeats)
        return 0
    rows = []
    for shape, (_, _, _, limit) in SHAPES.items():
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--shape", shape, "--repeats", str(args.repeats)],
                           capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.stderr.write("%s failed with status %d: stopping\n" % (shape, p.returncode))
            return p.returncode or 1
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    render(rows, args.out, args.repeats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
