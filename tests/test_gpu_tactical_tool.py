"""examples/ttt_tactical.py runs at a small batch (tools/tactical_rate.py: tests/test_gpu_rate_tools.py)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs(run_fresh):
    rc, out = run_fresh([sys.executable, "examples/ttt_tactical.py", "--batch", "512", "--playouts", "16"], cwd=ROOT, timeout=600)
    assert rc == 0, out[-3000:]
    assert out.count("against tactical") == 6 and "flat_mc tactical" in out, out[-2000:]
