"""examples/stats_overlaps.py (the reference's stats_overlaps comparison, scripts/scripts.jl:459-522) runs end to end at a toy size."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_stats_overlaps(capsys):
    spec = importlib.util.spec_from_file_location("stats_overlaps", os.path.join(ROOT, "examples", "stats_overlaps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows, mom = mod.main(["--N", "130", "--samples", "10", "--step", "300", "--replicas", "6", "--pairs", "2"])
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "#time self std cross std" and len(out) == len(rows) + 2 and len(rows) >= 2
    for t, s_m, s_s, x_m, x_s in rows:
        assert t >= 300 and 0.0 <= x_m <= 1.0 and 0.0 <= s_m <= 1.0 and s_s >= 0.0 and x_s >= 0.0
    # independent chains: the cross overlap stays below the self overlap of a chain with its own recent past
    assert rows[0][3] < rows[0][1]
    assert mom["pairs"] == 15 and 0.0 < mom["q2"] < 1.0 and mom["q4"] <= mom["q2"] and mom["binder"] <= 1.0
