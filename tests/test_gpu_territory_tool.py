"""tools/territory_rate.py runs end to end on the GPU (its --tiny shapes) and writes the rows DESIGN.md section 4.1b quotes."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_territory_rate_tool_smoke(tmp_path):
    out = tmp_path / "rate.jsonl"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "territory_rate.py"), "--tiny", "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["N"], row["B"], row["A"]) for row in rows] == [(19, 64, 3), (20, 64, 1)]
    every = {"N", "P", "B", "A", "ms", "instances_per_s", "mean_depth", "observe_all_ms", "sample_territory_ms", "sample_avoid_ms"}
    decision = {"decision_ms", "flat_mc_playouts", "flat_mc_ms", "decision_cheaper", "flat_mc_over_decision"}
    assert set(rows[0]) == every | decision and set(rows[1]) == every
    for row in rows:
        assert row["P"] == 4 and row["ms"] > 0 and row["instances_per_s"] > 0 and row["observe_all_ms"] > 0
        assert row["sample_territory_ms"] > 0 and row["sample_avoid_ms"] > 0
        assert 1 <= row["mean_depth"] <= row["N"] * row["N"]
    assert rows[0]["decision_ms"] > 0 and rows[0]["flat_mc_ms"] > 0 and rows[0]["flat_mc_playouts"] == 4
