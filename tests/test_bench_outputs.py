"""CPU tests of bench.py's --dump-outputs writer: float .npy files only, under 64 MB in all at any replica count, the same seeded sample of
replicas in every run, configurations unpacked in graphs.Config's bit layout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _results(R, samples, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.integers(-6144, 6145, (R, samples), dtype=np.int64), rng.integers(0, 1 << 22, R, dtype=np.int64),
            rng.integers(0, 2**63, (R, (bench.N_SITES + 63) // 64), dtype=np.uint64))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_default_shape_keeps_every_chain(pkg, tmp_path):
    Es, acc, s = _results(bench.REPLICAS_PER_GPU, bench.ITERS // bench.SAMPLE_STEP)
    bench.dump_outputs(str(tmp_path), Es, acc, s, 0)
    got = _load(str(tmp_path))
    assert set(got) == {"energies", "accepted", "energies_replicas", "spins", "spins_replicas"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 * 10**6
    assert (got["energies"] == Es).all() and (got["accepted"] == acc).all()
    assert (got["energies_replicas"] == np.arange(len(acc))).all()
    ids = got["spins_replicas"].astype(np.int64)
    assert len(ids) == bench.DUMP_SPIN_REPLICAS and (np.diff(ids) > 0).all()
    assert (got["spins"] == 2 * pkg.Config(bench.N_SITES, len(ids), s[ids]).bits().astype(np.float32) - 1).all()


def test_dump_outputs_samples_large_jobs_the_same_way_every_run(tmp_path):
    Es, acc, s = _results(20000, 1024)          # above DUMP_CHAIN_BYTES // (4 * 1024 + 16) = 10 700 replicas: sampled (160 MB of input)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, Es, acc, s, 4096)
    bench.dump_outputs(b, Es, acc, s, 4096)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 10**6
    ga, gb = _load(a), _load(b)
    assert all((ga[k] == gb[k]).all() for k in ga)
    rows = ga["energies_replicas"].astype(np.int64) - 4096
    assert 0 < len(rows) < len(acc) and (ga["energies"] == Es[rows]).all() and (ga["accepted"] == acc[rows]).all()
