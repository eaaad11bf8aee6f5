"""tools/mcts_agent_rate.py runs end to end on the GPU (its --tiny shape) and writes the rows DESIGN.md quotes;
examples/ttt_search_opponent.py runs at a small batch."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mcts_agent_rate_tool_smoke(tmp_path, run_fresh):
    out = tmp_path / "rate.jsonl"
    rc, log = run_fresh([sys.executable, os.path.join(ROOT, "tools", "mcts_agent_rate.py"), "--tiny", "--out", str(out)], cwd=ROOT,
                        timeout=600)
    assert rc == 0, log[-3000:]
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["shape"], row["B"], row["S"], row["R"]) for row in rows] == [("3x3_k3_p2", 64, 16, 4)]
    for row in rows:
        assert row["step_single_mcts_ms"] > 0 and row["mcts_ms"] > 0 and row["step_single_random_ms"] > 0
        assert 0 < row["searches_per_call"] <= 2 and row["ms_per_search"] > 0       # P = 2: at most 2 (P - 1) opponent plies
        assert abs(row["floor_ms"] - (row["mcts_ms"] + row["step_single_random_ms"])) < 1e-3 and row["step_over_floor"] > 0
        assert row["rollout_plies"] == 2 and row["rollout_mcts_ms"] > 0 and row["rollout_plies_per_s"] > 0


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/ttt_search_opponent.py", "--batch", "256", "--simulations", "16", "--playouts", "4"],
                        cwd=ROOT, timeout=600)
    assert rc == 0, out[-3000:]
    assert out.count("against mcts,") == 6 and out.count("against tactical,") == 6 and out.count("against random,") == 6, out[-2000:]
    assert out.count("self-play of the search") == 1
