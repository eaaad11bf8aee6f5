"""tools/blokus_puct_rate.py runs end to end on the GPU at its --tiny size, in a fresh process, and writes the rows DESIGN.md
quotes (as tests/test_gpu_tron_puct_tool.py does for its sibling); examples/blokus_puct.py runs at its --tiny size."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blokus_puct_rate_tool(tmp_path, run_fresh):
    out = tmp_path / "rate.jsonl"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "blokus_puct_rate.py"), "--tiny", "--out", str(out)]
    rc, log, err = run_fresh(cmd, cwd=ROOT, timeout=120, split=True)
    assert rc == 0, (log + err)[-3000:]
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["B"], row["S"], row["W"]) for row in rows] == [(32, 8, 8)]
    for row in rows:
        for key in ("select_us", "backup_us", "pair_us", "puct_ms", "step_observe_us", "mcts_ms", "simulations_per_s",
                    "pair_over_two_step_observe"):
            assert row[key] > 0, (key, row)
        assert 2 <= row["mean_nodes"] <= row["S"] + 1 and 0 <= row["mean_depth_last"] <= row["S"]
        assert row["puct_ms"] * 1e3 >= row["S"] * row["pair_us"] * 0.5         # the whole search holds its S pairs


def test_blokus_puct_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/blokus_puct.py", "--tiny"], cwd=ROOT, timeout=180)
    assert rc == 0, out[-3000:]
    assert out.count("win share") == 2 and "puct" in out and "random" in out, out[-2000:]
