"""Every rate and A/B tool under tools/ that times GPU calls through tools/common/measure.py runs end to end on the GPU, each
in a fresh process (run_fresh), with its --tiny shapes or its smallest arguments, and writes the rows DESIGN.md quotes.
A run takes 2 to 4 s on an MI355X (the figure beside each); its limit is 60 s per process it starts, because the first import
of torch on a machine can take most of a minute (the runs had 600 s each before)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = "colosseumrl_amd/libcolosseum_hip.so"


def _tactical(rows, log):
    assert [(row["shape"], row["B"], row["playouts"], row["rounds"]) for row in rows] == [("3x3_k3_p2", 1024, 4096, 1),
                                                                                          ("3x5_k3_p3", 1024, 4096, 1)]
    for row in rows:
        for fig in ("step_single_us", "playout_plies_per_s", "rollout_env_steps_per_s"):
            for agent in ("random", "tactical"):
                lo, hi = row[fig + "_" + agent + "_spread"]
                assert 0 < lo <= row[fig + "_" + agent] <= hi
            assert row[fig + "_random_parent"] is None       # no --parent-lib: the parent's figures are not made up
        assert row["winning_cells_us"] > 0 and row["noise"] == 0.1
        assert row["step_single_tactical_over_random"] > 0 and row["playout_random_over_tactical"] > 0


def _mcts(rows, log):
    assert [(row["shape"], row["B"], row["S"], row["R"]) for row in rows] == [("3x3_k3_p2", 64, 16, 4)]
    for row in rows:
        assert row["mcts_ms"] > 0 and row["flat_mc_ms"] > 0 and row["simulations_per_s"] > 0
        assert row["flat_mc_playouts_per_position"] >= row["S"] * row["R"] >= row["playouts_per_position"] > 0
        assert row["plies_per_position"] >= row["playouts_per_position"] and row["playout_plies_per_s"] > 0
        assert 2 <= row["mean_nodes"] <= row["S"] + 1


def _mcts_agent(rows, log):
    assert [(row["shape"], row["B"], row["S"], row["R"]) for row in rows] == [("3x3_k3_p2", 64, 16, 4)]
    for row in rows:
        assert row["step_single_mcts_ms"] > 0 and row["mcts_ms"] > 0 and row["step_single_random_ms"] > 0
        assert 0 < row["searches_per_call"] <= 2 and row["ms_per_search"] > 0       # P = 2: at most 2 (P - 1) opponent plies
        assert abs(row["floor_ms"] - (row["mcts_ms"] + row["step_single_random_ms"])) < 1e-3 and row["step_over_floor"] > 0
        assert row["rollout_plies"] == 2 and row["rollout_mcts_ms"] > 0 and row["rollout_plies_per_s"] > 0


def _territory(rows, log):
    assert [(row["N"], row["B"], row["A"]) for row in rows] == [(19, 64, 3), (20, 64, 1)]
    every = {"N", "P", "B", "A", "ms", "instances_per_s", "mean_depth", "observe_all_ms", "sample_territory_ms", "sample_avoid_ms"}
    decision = {"decision_ms", "flat_mc_playouts", "flat_mc_ms", "decision_cheaper", "flat_mc_over_decision"}
    assert set(rows[0]) == every | decision and set(rows[1]) == every
    for row in rows:
        assert row["P"] == 4 and row["ms"] > 0 and row["instances_per_s"] > 0 and row["observe_all_ms"] > 0
        assert row["sample_territory_ms"] > 0 and row["sample_avoid_ms"] > 0
        assert 1 <= row["mean_depth"] <= row["N"] * row["N"]
    assert rows[0]["decision_ms"] > 0 and rows[0]["flat_mc_ms"] > 0 and rows[0]["flat_mc_playouts"] == 4


def _playout(rows, log):
    assert {row["game"] for row in rows} == {"tictactoe", "blokus"}
    assert all(row["playouts_per_s"] > 0 and row["plies_per_s"] > 0 for row in rows)


def _tron_playout(rows, log):
    assert {row["agent"] for row in rows} == {"random", "avoid"}
    assert all(row["playouts_per_s"] > 0 and row["steps_per_s"] > 0 and row["loop_ms"] > 0 for row in rows)


def _avoid(rows, log):
    assert [(row["N"], row["B"], row["T"]) for row in rows] == [(19, 256, 4)]
    assert rows[0]["fused_equals_loop"] is True              # (exit 0, asserted for every tool, says the same)


def _single(rows, log):
    assert [row["game"] for row in rows] == ["ttt_3x3_k3_p2", "ttt_3x5_k3_p3", "ttt_3x3x3_k3_p4", "blokus"]
    for row in rows:
        assert all(row[key] > 0 for key in row if "_us_" in key), row


def _step_api(rows, log):
    assert len([ln for ln in log.splitlines() if "/s" in ln]) == 9, log[-3000:]


def _lib_ab(rows, log):
    lines = [ln for ln in log.splitlines() if ln.startswith("tron_p4_n20_b65536 T=20 ")]
    assert [ln.split()[2] for ln in lines] == ["one", "two"], log[-3000:]
    assert all("env-steps/s" in ln and float(ln.split()[4]) > 0 for ln in lines)


# (tool, arguments, whether it takes --out, time limit in s, the check of its rows / its output); beside each the seconds
# the run took on an MI355X
TOOLS = [
    ("tactical_rate.py", ["--tiny"], True, 120, _tactical),                                                  # 2.1 (two starts)
    ("mcts_rate.py", ["--tiny"], True, 120, _mcts),                                                          # 2.2
    ("mcts_agent_rate.py", ["--tiny"], True, 120, _mcts_agent),                                              # 2.1
    ("territory_rate.py", ["--tiny"], True, 120, _territory),                                                # 2.1
    ("playout_rate.py", ["--tiny"], True, 120, _playout),                                                    # 2.7
    ("tron_playout_rate.py", ["--tiny"], True, 120, _tron_playout),                                          # 2.1
    ("avoid_rate.py", ["--batch", "256", "--sizes", "19", "--steps", "4", "--reps", "1"], True, 120, _avoid),                    # 2.2
    ("single_rate.py", ["--blokus-batch", "64", "--ttt-batch", "1024", "--steps", "2", "--reps", "1"], True, 120, _single),      # 2.1
    ("step_api_rate.py", [], False, 120, _step_api),                                                         # 2.2
    # the only 20x20 P4 workload, one launch length, both tags the shipped library
    ("lib_ab.py", ["--rounds", "1", "tron_p4_n20_b65536", "20", "one=" + LIB, "two=" + LIB], False, 180, _lib_ab),               # 4.1 (three starts)
]


@pytest.mark.parametrize("tool,args,takes_out,limit,check", TOOLS, ids=[t[0][:-3] for t in TOOLS])
def test_rate_tool(tmp_path, run_fresh, tool, args, takes_out, limit, check):
    out = tmp_path / "rate.jsonl"
    cmd = [sys.executable, os.path.join(ROOT, "tools", tool)] + args + (["--out", str(out)] if takes_out else [])
    rc, log, err = run_fresh(cmd, cwd=ROOT, timeout=limit, split=True)
    assert rc == 0, (log + err)[-3000:]
    check([json.loads(line) for line in out.read_text().splitlines()] if takes_out else None, log)
