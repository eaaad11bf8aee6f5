"""examples/ttt_search_opponent.py runs at a small batch (tools/mcts_agent_rate.py: tests/test_gpu_rate_tools.py)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/ttt_search_opponent.py", "--batch", "256", "--simulations", "16", "--playouts", "4"],
                        cwd=ROOT, timeout=600)
    assert rc == 0, out[-3000:]
    assert out.count("against mcts,") == 6 and out.count("against tactical,") == 6 and out.count("against random,") == 6, out[-2000:]
    assert out.count("self-play of the search") == 1
