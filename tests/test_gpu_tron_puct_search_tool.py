"""tools/tron_search_rate.py runs end to end on the GPU at its --tiny size, in a fresh process, and writes the row the README
quotes (as tests/test_gpu_tron_net_tool.py does for its sibling)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tron_search_rate_tool(tmp_path, run_fresh):
    out = tmp_path / "rate.jsonl"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "tron_search_rate.py"), "--tiny", "--out", str(out)]
    rc, log, err = run_fresh(cmd, cwd=ROOT, timeout=120, split=True)
    assert rc == 0, (log + err)[-3000:]
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["shape"], row["B"], row["S"]) for row in rows] == [("7x7_p2", 64, 8)]
    for row in rows:
        for key in ("loop_sim_us", "fused_sim_us", "loop_over_fused"):
            assert row[key] > 0, (key, row)
        assert row["network"]["inputs"] == 200 and row["network"]["hidden"] == 32
        for way in ("loop", "fused"):
            lo, hi = row[way + "_sim_range_us"]
            assert lo <= row[way + "_sim_us"] <= hi
        assert isinstance(row["fused_faster_beyond_spread"], bool) and row["same_root"] is True
