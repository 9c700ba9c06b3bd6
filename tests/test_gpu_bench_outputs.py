"""A plain `bench.py` run on hardware: the line holds the headline and nothing that takes runs of its own (those come with --full), and
--dump-outputs writes what the last timed step computed — checked against the oracle's chains from the initial spins through the warm-up
and every timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_the_last_step(pkg, oracle, tmp_path):
    import bench
    R, iters, steps, warmup = 256, 1 << 14, 3, 1
    out = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--iters", str(iters), "--replicas", str(R), "--dump-outputs", out], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, RRRMC_BENCH_DETAIL=str(tmp_path / "detail.json")))
    assert r.returncode == 0, r.stderr
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["roofline"]["launches"] > 0 and line["verified"] is None
    assert not {"secondary", "cpu_baseline", "sync_value"} & set(line)
    E, acc = np.load(os.path.join(out, "energies.npy")), np.load(os.path.join(out, "accepted.npy"))
    spins, ids = np.load(os.path.join(out, "spins.npy")), np.load(os.path.join(out, "spins_replicas.npy")).astype(np.int64)
    assert E.shape == (R, iters // bench.SAMPLE_STEP) and acc.shape == (R,) and spins.shape == (R, bench.N_SITES)
    assert (np.load(os.path.join(out, "energies_replicas.npy")) == np.arange(R)).all() and (ids == np.arange(R)).all()
    X = pkg.GraphRRG(bench.N_SITES, bench.K_DEG, seed=bench.SEED)
    A, J = X.A, X.J.astype(np.int32)
    for rep in (0, R // 2, R - 1):
        ch = oracle.init_configs(bench.SEED, rep, 1, bench.N_SITES)[0]
        ch = oracle.standard_mc_sparse(A, J, bench.BETA, iters * (warmup + steps - 1), bench.SAMPLE_STEP, bench.SEED, ch, replica=rep)[1]
        Es_ref, ch_ref, acc_ref = oracle.standard_mc_sparse(A, J, bench.BETA, iters, bench.SAMPLE_STEP, bench.SEED, ch,
                                                            it0=iters * (warmup + steps - 1), replica=rep)[:3]
        assert (E[rep] == Es_ref).all() and acc[rep] == acc_ref
        assert (spins[rep] == 2 * pkg.Config(bench.N_SITES, 1, ch_ref[None]).bits()[0].astype(np.float32) - 1).all()
