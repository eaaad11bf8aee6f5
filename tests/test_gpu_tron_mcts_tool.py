"""tools/tron_mcts_rate.py with its --tiny shapes and examples/tron_mcts.py at a small batch, each end to end in a fresh
process."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rate_tool_runs(run_fresh, tmp_path):
    out_path = str(tmp_path / "tron_mcts_rate.jsonl")
    rc, out = run_fresh([sys.executable, "tools/tron_mcts_rate.py", "--tiny", "--out", out_path], cwd=ROOT, timeout=120)
    assert rc == 0, out[-3000:]
    rows = [json.loads(line) for line in open(out_path)]
    assert [(r["N"], r["P"], r["B"], r["S"], r["R"], r["agent"]) for r in rows] == [(9, 4, 64, 16, 4, "random"), (9, 4, 64, 16, 4, "avoid")]
    for r in rows:
        assert r["mcts_ms"] > 0 and r["flat_mc_ms"] > 0 and r["simulations_per_s"] > 0 and r["mcts_over_flat_mc_time"] > 0
        assert r["flat_mc_playouts_per_position"] >= r["S"] * r["R"] >= r["playouts_per_position"] >= 0
        assert 2 <= r["mean_nodes"] <= r["S"] + 1 and 1 <= r["mean_depth"] <= r["S"]
        assert r["playout_steps_per_position"] >= r["playouts_per_position"]


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/tron_mcts.py", "--batch", "128", "--simulations", "12", "--playouts", "4"],
                        cwd=ROOT, timeout=120)
    assert rc == 0, out[-3000:]
    lines = [ln.split() for ln in out.splitlines()]
    assert [ln[0] for ln in lines if ln and ln[0] in ("mcts", "territory", "flat", "avoid", "random")] == \
        ["mcts", "territory", "flat", "avoid", "random"], out[-2000:]
    win = {ln[0]: float(ln[-1]) for ln in lines if ln and ln[0] in ("mcts", "random")}
    assert 0.0 <= win["random"] <= win["mcts"] <= 1.0, out[-2000:]
