"""examples/ttt_mcts.py runs at a small batch (tools/mcts_rate.py: tests/test_gpu_rate_tools.py)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/ttt_mcts.py", "--batch", "256", "--simulations", "32", "--playouts", "4"],
                        cwd=ROOT, timeout=600)
    assert rc == 0, out[-3000:]
    assert out.count("mcts") == 6 and out.count("against tactical") == 9 and out.count("against random") == 9, out[-2000:]
