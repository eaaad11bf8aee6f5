"""examples/blokus_search_opponent.py and tools/blokus_mcts_agent_rate.py run end to end on the GPU at their smallest sizes
(--tiny), each in a fresh process (run_fresh)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/blokus_search_opponent.py", "--tiny"], cwd=ROOT, timeout=120)
    assert rc == 0, out[-3000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("blokus, against 3 x ") and "learner" in ln]
    assert len(lines) == 30 and sum(" games)" in ln for ln in lines) == 24, out[-2000:]
    assert all(8 <= int(ln.split("(")[1].split()[0]) <= 16 for ln in lines if " games)" in ln), out[-2000:]   # first episodes finished
    for opponent in ("random", "mcts"):
        for learner in ("random", "flat_mc", "mcts"):
            assert sum(("3 x %-6s: %-7s learner" % (opponent, learner)) in ln for ln in lines) == 5, out[-2000:]
    for ln in lines:
        share, rank = float(ln.split("win share ")[1].split()[0]), float(ln.split("mean final rank ")[1].split()[0])
        assert 0.0 <= share <= 1.0 and 0.0 <= rank <= 3.0, ln


def test_rate_tool_runs(tmp_path, run_fresh):
    """--tiny: 32 positions, 8 simulations, W = 4, R = 1 (a wave per game) and 4 (a workgroup per game), 2 rollout plies; the
    tool itself stops unless sample_mcts is mcts's best everywhere and the restatement reproduces the sampled game"""
    out = tmp_path / "rate.jsonl"
    rc, log, err = run_fresh([sys.executable, os.path.join(ROOT, "tools", "blokus_mcts_agent_rate.py"), "--tiny", "--out", str(out)],
                             cwd=ROOT, timeout=120, split=True)
    assert rc == 0, (log + err)[-3000:]
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["B"], row["S"], row["W"], row["R"], row["mapping"]) for row in rows] == [(32, 8, 4, 1, "wave per game"),
                                                                                         (32, 8, 4, 4, "workgroup per game")]
    for row in rows:
        for k in ("mcts_ms", "sample_ms", "step_ms", "step_random_ms", "rollout_ms"):
            assert row[k] > 0, k
        for k in ("mcts_ms", "sample_ms", "step_ms", "rollout_ms"):
            lo, hi = row[k + "_range"]
            assert 0 < lo <= row[k] <= hi, k
        assert abs(row["floor_ms"] - (3 * row["mcts_ms"] + row["step_random_ms"])) < 1e-3
        assert row["sample_over_mcts"] > 0 and row["step_over_floor"] > 0 and row["noise"] == 0.0
        assert 3.0 <= row["opponent_plies_per_game"] <= 6.0 and 0 <= row["searches_in_sampled_games"] <= 6
        assert row["rollout_plies"] == 2 and row["rollout_plies_per_s"] > 0
