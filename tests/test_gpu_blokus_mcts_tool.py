"""examples/blokus_mcts.py and tools/blokus_mcts_rate.py run end to end on the GPU at their smallest sizes (--tiny), each in
a fresh process (run_fresh)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/blokus_mcts.py", "--tiny"], cwd=ROOT, timeout=120)
    assert rc == 0, out[-3000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("blokus, ") and "learner" in ln]
    assert len(lines) == 15 and sum(" games)" in ln for ln in lines) == 12, out[-2000:]
    assert all(8 <= int(ln.split("(")[1].split()[0]) <= 16 for ln in lines if " games)" in ln), out[-2000:]   # first episodes finished
    for learner in ("random", "flat_mc", "mcts"):
        assert sum((learner + " ") in ln for ln in lines) == 5, out[-2000:]
    for ln in lines:
        share, rank = float(ln.split("win share ")[1].split()[0]), float(ln.split("mean final rank ")[1].split()[0])
        assert 0.0 <= share <= 1.0 and 0.0 <= rank <= 3.0, ln


def test_rate_tool_runs(tmp_path, run_fresh):
    """--tiny: 32 positions, 8 simulations, W = 4, R = 1 (a wave per tree) and 4 (a workgroup per tree); the tool itself
    stops unless the restatement's tree on the sampled position is the kernel's"""
    out = tmp_path / "rate.jsonl"
    rc, log, err = run_fresh([sys.executable, os.path.join(ROOT, "tools", "blokus_mcts_rate.py"), "--tiny", "--out", str(out)],
                             cwd=ROOT, timeout=120, split=True)
    assert rc == 0, (log + err)[-3000:]
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["B"], row["S"], row["W"], row["R"], row["mapping"]) for row in rows] == [(32, 8, 4, 1, "wave per tree"),
                                                                                         (32, 8, 4, 4, "workgroup per tree")]
    for row in rows:
        assert row["mcts_ms"] > 0 and row["flat_mc_ms"] > 0 and row["simulations_per_s"] > 0 and row["mcts_over_flat_mc_time"] > 0
        assert row["flat_mc_playouts_per_position"] == row["S"] * row["R"] >= row["playouts_per_position"] > 0
        assert row["plies_per_position"] >= row["playouts_per_position"] and row["playout_plies_per_s"] > 0
        assert 2 <= row["mean_nodes"] <= row["S"] + 1
