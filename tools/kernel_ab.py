#!/usr/bin/env python3
"""A/B of the interchangeable Tron rollout kernels on one device (interleaved rounds in one process):
python3 tools/kernel_ab.py [N] [steps per launch]"""
import os
import sys
if "-h" in sys.argv[1:] or "--help" in sys.argv[1:]:     # usage without touching the GPU (tests/test_tools_smoke.py)
    print(__doc__)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools.common import measure as M
from colosseumrl_amd.batched import TronBatch

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
T = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
B = 65536
tbs = {k: TronBatch(N, 4, B) for k in (("quad", "bytes", "bits", "qbits") if N <= 20 else ("bytes", "bits", "qbits"))}
for k, tb in tbs.items():
    tb.rollout(T, 0, kernel=k)
res = {k: [] for k in tbs}
for rnd in range(5):                                     # (the kernels take turns: a round of each, five times)
    for k, tb in tbs.items():
        res[k] += M.back_to_back(lambda: tb.rollout(T, 0, kernel=k), calls=3, rounds=1)
for k, v in res.items():
    print("N=%d T=%d %-5s median %.3f ms  min %.3f ms  -> %.4g env-steps/s" % (N, T, k, M.median(v), min(v), B * T / (M.median(v) * 1e-3)))
for k in tbs:
    assert torch.equal(tbs["bytes"].board, tbs[k].board) and torch.equal(tbs["bytes"].ret_sum, tbs[k].ret_sum), k
