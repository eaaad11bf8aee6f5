#!/usr/bin/env python3
"""Throughput of a workload's rollout kernel against the batch size (= resident waves per SIMD): is the kernel bound by
instruction issue (throughput flat beyond the workload's own batch) or by the latency of its dependent chains (throughput
rises with more waves per SIMD)?
    python tools/debug/batch_sweep.py <workload> <steps per launch> <batch>[,<batch>...]"""
import os
import sys
if "-h" in sys.argv[1:] or "--help" in sys.argv[1:]:     # usage without touching the GPU (tests/test_tools_smoke.py)
    print(__doc__)
    sys.exit(0)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import bench
from tools.common import measure as M

wl, T = sys.argv[1], int(sys.argv[2])
game, kw = bench.WORKLOADS[wl][:2]
for B in [int(x) for x in sys.argv[3].split(",")]:
    st = bench.make_stepper(game, kw, B, torch.device("cuda", 0), 0)
    ms = M.median(M.back_to_back(lambda: st.rollout(T, 0), calls=10, rounds=5, warmup=3))
    print("%s T=%d B=%-8d %8.4f ms per launch  %.4g env-steps/s" % (wl, T, B, ms, B * T / (ms * 1e-3)), flush=True)
    del st
