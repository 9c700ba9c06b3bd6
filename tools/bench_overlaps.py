"""Cross-replica overlaps on the device against what a user did before them: `Engine.overlap_hist` on one same-slot pair and
`Engine.cross_overlaps` on a 1024 x 1024 block, beside `snapshot_get` + numpy xor / popcount on the host (one thread) for the same pairs.

  python tools/bench_overlaps.py [--out profiles/r21/cross_overlaps.md] [--repeats 5]

Without --shape the script starts one child process per shape, each under its own `timeout`, one after the other, and stops at the
first that fails; it never opens the device itself.  Each child warms every call up, repeats it, and prints one JSON line with the
medians.  The parent renders the lines into the Markdown file, stamped with the sources they were measured on.
Call times are host clocks around calls that end in a device synchronise (both calls return results to the host)."""
import argparse
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
    "rrg4096_r1024": ("GraphRRG", 4096, 1024, 240),
    "rrg4096_r8192": ("GraphRRG", 4096, 8192, 420),
    "sk1024_r2048": ("GraphSK", 1024, 2048, 300),
}
SOURCES = ["rrrmc.jl_amd/csrc/xov_kernels.hpp", "rrrmc.jl_amd/csrc/xov_core.hpp", "rrrmc.jl_amd/csrc/host_xov.hpp", "rrrmc.jl_amd/csrc/layout_kernels.hpp"]
BLOCK = 1024


def _median_ms(fn, repeats):
    fn()                                                     # warm-up: code objects, buffers grown on demand
    t0 = time.perf_counter()
    fn()
    n = max(1, min(500, int(0.25 / max(time.perf_counter() - t0, 1e-6))))     # a timed sample is n calls, about a quarter of a second
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        ts.append((time.perf_counter() - t0) * 1e3 / n)
    return statistics.median(ts), min(ts), max(ts)


def host_hist(chunks, N):
    """numpy on one thread: Hamming distances of every r1 < r2, in stripes of rows"""
    R = chunks.shape[0]
    h = np.zeros(N + 1, np.int64)
    stripe = max(1, (1 << 23) // max(R * chunks.shape[1], 1))              # 64 MiB of xor words at a time
    for i0 in range(0, R, stripe):
        a = chunks[i0:i0 + stripe]
        d = np.bitwise_count(a[:, None, :] ^ chunks[None, i0:, :]).sum(axis=2, dtype=np.int64)        # [stripe, R - i0]
        keep = np.arange(i0, R)[None, :] > np.arange(i0, i0 + a.shape[0])[:, None]
        h += np.bincount(d[keep], minlength=N + 1)
    return h


def host_block(chunksA, chunksB, N):
    q = np.empty((chunksA.shape[0], chunksB.shape[0]), np.int32)
    for i0 in range(0, chunksA.shape[0], 64):
        d = np.bitwise_count(chunksA[i0:i0 + 64, None, :] ^ chunksB[None, :, :]).sum(axis=2, dtype=np.int64)
        q[i0:i0 + 64] = N - 2 * d
    return q


def run_shape(name, repeats):
    import __graft_entry__ as e
    pkg = e.load_package()
    if pkg.lib().rrrmc_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    graph, N, R, _ = SHAPES[name]
    X = pkg.GraphRRG(N, 3, seed=8370000274) if graph == "GraphRRG" else pkg.GraphSK(N, seed=8370000274)
    nch = (N + 63) // 64
    nb = min(BLOCK, R)
    with pkg.Engine(X, R) as eng:
        eng.seed(6540000789)
        eng.init_spins_random()
        eng.snapshot_reserve(2)
        for k in range(2):
            eng.standard_mc(1.0, 4 * N, 4 * N)
            eng.snapshot_store(k)
        rec = {"shape": name, "graph": "%s(%d%s)" % (graph, N, ", 3" if graph == "GraphRRG" else ""), "N": N, "R": R, "nch": nch, "repeats": repeats}
        rec["pack_ms"] = _median_ms(lambda: eng.cross_overlaps(0, 0, rowsA=(0, 1), rowsB=(0, 1)), repeats)      # one slot packed, one 1 x 1 block
        rec["hist_ms"] = _median_ms(lambda: eng.overlap_hist(0, 0), repeats)
        rec["block_ms"] = _median_ms(lambda: eng.cross_overlaps(0, 1, rowsA=(0, nb), rowsB=(R - nb, nb)), repeats)
        h_dev = eng.overlap_hist(0, 0)
        q_dev = eng.cross_overlaps(0, 1, rowsA=(0, nb), rowsB=(R - nb, nb))[0]
        # the host path, once (it takes seconds): fetch the snapshots, then xor / popcount in numpy
        t0 = time.perf_counter()
        c0, c1 = eng.snapshot_get(0).s, eng.snapshot_get(1).s
        rec["host_get_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    h_host = host_hist(c0, N)
    rec["host_hist_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    q_host = host_block(c0[:nb], c1[R - nb:], N)
    rec["host_block_ms"] = (time.perf_counter() - t0) * 1e3
    if not (h_dev == h_host).all() or not (q_dev == q_host).all():
        raise SystemExit("%s: the device results differ from the host path" % name)
    rec["hist_pair_words"] = R * (R - 1) // 2 * nch
    rec["block_pair_words"] = nb * nb * nch
    print(json.dumps(rec), flush=True)


def render(recs, path):
    import bench
    lines = ["# Cross-replica overlaps: device calls against the host path", "",
             "source_stamp: %s (%s)" % (bench.source_stamp(SOURCES), ", ".join(SOURCES)), "git_commit: %s" % (bench.git_head() or "unknown"),
             "", "Measured by `tools/bench_overlaps.py` on one MI355X: ms per call, medians of %d timed samples after a warm-up call (min .. max in brackets); a sample is about a quarter of a" % recs[0]["repeats"],
             "second of back-to-back calls under a host clock, and every call ends in a device synchronise.  The host path is `snapshot_get` of the slots plus numpy xor / `bitwise_count` on one thread, run once.",
             "A pair-word is one 64-bit xor + popcount of one replica pair.  The device results were compared with the host path's in the same run: equal.", "",
             "| shape | call | device ms | pair-words/s | host path ms (get + numpy) | host / device | pack share |", "|---|---|---|---|---|---|---|"]
    for r in recs:
        for call, key, words, host in (("overlap_hist, one same-slot pair", "hist_ms", r["hist_pair_words"], r["host_get_ms"] / 2 + r["host_hist_ms"]),
                                       ("cross_overlaps, %d x %d block" % ((min(BLOCK, r["R"]),) * 2), "block_ms", r["block_pair_words"], r["host_get_ms"] + r["host_block_ms"])):
            med, lo, hi = r[key]
            lines.append("| %s, R = %d | %s | %.3f (%.3f .. %.3f) | %.3g | %.1f | %.0f x | %.0f %% |"
                         % (r["graph"], r["R"], call, med, lo, hi, words / (med * 1e-3), host, host / med, 100.0 * min(1.0, r["pack_ms"][0] / med)))
    lines += ["", "Pack share: the median time of a call that packs one slot and computes a single 1 x 1 block (%s ms for the shapes above, in order) over the"
              % ", ".join("%.3f" % r["pack_ms"][0] for r in recs),
              "call's time: the packing, the table upload, the launch and the result copy — everything but the tiles.  A call that names two slots packs twice."]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "cross_overlaps.md"))
    a = ap.parse_args()
    if a.shape:
        return run_shape(a.shape, a.repeats)
    recs = []
    for name, (_, _, _, limit) in SHAPES.items():            # one child per shape, under its own time limit; the first failure ends the script
        out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--shape", name, "--repeats", str(a.repeats)],
                             capture_output=True, text=True)
        sys.stderr.write(out.stderr[-2000:])
        if out.returncode != 0:
            raise SystemExit("%s: exit status %d: stopping" % (name, out.returncode))
        recs.append(json.loads(out.stdout.strip().splitlines()[-1]))
        print(json.dumps(recs[-1]), flush=True)
    render(recs, a.out)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
