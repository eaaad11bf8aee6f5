"""tools/tactical_rate.py runs end to end on the GPU (its --tiny shapes) and writes the rows DESIGN.md quotes;
examples/ttt_tactical.py runs at a small batch."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tactical_rate_tool_smoke(tmp_path):
    out = tmp_path / "rate.jsonl"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tactical_rate.py"), "--tiny", "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["shape"], row["B"], row["playouts"], row["rounds"]) for row in rows] == [("3x3_k3_p2", 1024, 4096, 1),
                                                                                          ("3x5_k3_p3", 1024, 4096, 1)]
    for row in rows:
        for fig in ("step_single_us", "playout_plies_per_s", "rollout_env_steps_per_s"):
            for agent in ("random", "tactical"):
                lo, hi = row[fig + "_" + agent + "_spread"]
                assert 0 < lo <= row[fig + "_" + agent] <= hi
            assert row[fig + "_random_parent"] is None       # no --parent-lib: the parent's figures are not made up
        assert row["winning_cells_us"] > 0 and row["noise"] == 0.1
        assert row["step_single_tactical_over_random"] > 0 and row["playout_random_over_tactical"] > 0


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/ttt_tactical.py", "--batch", "512", "--playouts", "16"], cwd=ROOT, timeout=600)
    assert rc == 0, out[-3000:]
    assert out.count("against tactical") == 6 and "flat_mc tactical" in out, out[-2000:]
