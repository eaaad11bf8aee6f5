"""tools/mcts_rate.py runs end to end on the GPU (its --tiny shape) and writes the rows DESIGN.md quotes;
examples/ttt_mcts.py runs at a small batch."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mcts_rate_tool_smoke(tmp_path, run_fresh):
    out = tmp_path / "rate.jsonl"
    rc, log = run_fresh([sys.executable, os.path.join(ROOT, "tools", "mcts_rate.py"), "--tiny", "--out", str(out)], cwd=ROOT,
                        timeout=600)
    assert rc == 0, log[-3000:]
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["shape"], row["B"], row["S"], row["R"]) for row in rows] == [("3x3_k3_p2", 64, 16, 4)]
    for row in rows:
        assert row["mcts_ms"] > 0 and row["flat_mc_ms"] > 0 and row["simulations_per_s"] > 0
        assert row["flat_mc_playouts_per_position"] >= row["S"] * row["R"] >= row["playouts_per_position"] > 0
        assert row["plies_per_position"] >= row["playouts_per_position"] and row["playout_plies_per_s"] > 0
        assert 2 <= row["mean_nodes"] <= row["S"] + 1


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/ttt_mcts.py", "--batch", "256", "--simulations", "32", "--playouts", "4"],
                        cwd=ROOT, timeout=600)
    assert rc == 0, out[-3000:]
    assert out.count("mcts") == 6 and out.count("against tactical") == 9 and out.count("against random") == 9, out[-2000:]
