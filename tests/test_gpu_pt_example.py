"""examples/pt_ea.py (parallel tempering on GraphEANormal beside a run at the coldest beta alone) runs end to end at a toy size."""
import importlib.util
import math
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_pt_ea(capsys):
    spec = importlib.util.spec_from_file_location("pt_ea", os.path.join(ROOT, "examples", "pt_ea.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows, trips, alone = mod.main(["--L", "4", "--betas", "0.3,0.6,0.9", "--replicas", "10", "--rounds", "30"])
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "#beta accept_next <E>/N <q^2> Binder" and len(out) == len(rows) + 4 and len(rows) == 3 and out[4].startswith("(accept_next")
    for k, (beta, acc, e, q2, binder) in enumerate(rows):
        assert (math.isnan(acc) if k == 2 else 0.0 < acc <= 1.0) and -3.0 < e < 0.0 and 0.0 <= q2 <= 1.0 and binder <= 1.0
    assert rows[0][2] > rows[2][2]                               # the hot end holds more energy than the cold end
    assert trips >= 0 and alone[0] == 0.9 and -3.0 < alone[1] < 0.0
