"""tools/tron_puct_rate.py runs end to end on the GPU at its --tiny size, in a fresh process, and writes the rows DESIGN.md
quotes (as tests/test_gpu_puct_tool.py does for its sibling); examples/tron_alphazero.py runs two tiny iterations."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tron_puct_rate_tool(tmp_path, run_fresh):
    out = tmp_path / "rate.jsonl"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "tron_puct_rate.py"), "--tiny", "--out", str(out)]
    rc, log, err = run_fresh(cmd, cwd=ROOT, timeout=120, split=True)
    assert rc == 0, (log + err)[-3000:]
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["N"], row["P"], row["B"], row["S"]) for row in rows] == [(9, 4, 64, 16)]
    for row in rows:
        for key in ("select_us", "backup_us", "pair_us", "root_us", "puct_ms", "step_observe_us", "mcts_territory_ms",
                    "simulations_per_s", "pair_over_two_step_observe"):
            assert row[key] > 0, (key, row)
        assert 1 <= row["searched_trees"] <= row["B"] and 2 <= row["mean_nodes"] <= row["S"] + 1
        assert 0 <= row["mean_depth_last"] <= row["S"]
        assert row["puct_ms"] * 1e3 >= row["S"] * row["pair_us"] * 0.5        # the whole search holds its S pairs


def test_tron_alphazero_example_runs(run_fresh):
    """two tiny iterations: it finishes, prints both win rates and the shapes of what it trained on"""
    cmd = [sys.executable, "examples/tron_alphazero.py", "--size", "7", "--players", "3", "--batch", "64", "--iterations", "2",
           "--simulations", "6", "--eval-games", "64", "--max-steps", "40"]
    rc, out = run_fresh(cmd, cwd=ROOT, timeout=180)
    assert rc == 0, out[-3000:]
    assert out.count("win rate against 2 avoid opponents") == 2 and "before" in out and "after 2 iterations" in out, out[-2000:]
    shapes = [ln for ln in out.splitlines() if ln.startswith("iteration")]
    assert len(shapes) == 2 and all("boards (" in ln and ", 49)" in ln and ", 3)" in ln and "values (" in ln for ln in shapes), out[-2000:]
