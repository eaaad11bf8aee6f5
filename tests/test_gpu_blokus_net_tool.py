"""tools/blokus_net_rate.py runs end to end on the GPU at its --tiny size, in a fresh process, and writes the two rows the README
quotes (as tests/test_gpu_tron_net_tool.py does for its sibling)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blokus_net_rate_tool(tmp_path, run_fresh):
    out = tmp_path / "rate.jsonl"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "blokus_net_rate.py"), "--tiny", "--out", str(out)]
    rc, log, err = run_fresh(cmd, cwd=ROOT, timeout=120, split=True)
    assert rc == 0, (log + err)[-3000:]
    rows = [json.loads(line) for line in out.read_text().splitlines()]
    assert [(row["B"], row["W"], row["S"]) for row in rows] == [(32, 4, 4), (32, 8, 4)]
    for row in rows:
        for key in ("torch_sim_us", "hip_sim_us", "net_eval_us", "pair_us", "pack_us"):
            assert row[key] > 0, (key, row)
        assert row["network"]["inputs"] == 1684 and row["network"]["hidden"] == 32
        assert row["hip_sim_range_us"][0] <= row["hip_sim_us"] <= row["hip_sim_range_us"][1]
        assert row["hip_sim_us"] >= 0.5 * row["pair_us"]                 # a simulation holds its select and backup
