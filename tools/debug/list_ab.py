#!/usr/bin/env python3
"""A/B of blokus_list_kernel builds on the GPU box: one child process per library (CRL_LIB_PATH), each times valid_list on the
16,384 mid-game positions bench.py uses and prints a hash of the lists, to hold against the first library's.
usage: python tools/debug/list_ab.py <lib.so> [<lib.so> ...]"""
import json
import os
import sys
if "-h" in sys.argv[1:] or "--help" in sys.argv[1:]:     # usage without touching the GPU (tests/test_tools_smoke.py)
    print(__doc__)
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402


def child():
    """one library: [median us, min us, mean legal moves, hash of the lists] as a JSON line behind "LIST " """
    import hashlib
    from colosseumrl_amd.batched import BlokusBatch
    bb = BlokusBatch(16384)
    bb.rollout(24, 5)
    count, ids = bb.valid_list(2048)
    ts = M.back_to_back(lambda: bb.valid_list(2048, out=ids), calls=20, rounds=5, warmup=5)
    h = hashlib.sha1(ids.cpu().numpy().tobytes() + count.cpu().numpy().tobytes()).hexdigest()[:12]
    print("LIST " + json.dumps([M.median(ts) * 1e3, min(ts) * 1e3, count.float().mean().item(), h]))


if sys.argv[1:] == ["--child"]:
    child()
else:
    libs = [(os.path.relpath(lib, ROOT), lib) for lib in sys.argv[1:]]
    for tag, result in M.alternate([sys.executable, os.path.abspath(__file__), "--child"], libs, 1, 600, "LIST "):
        print("%-40s %7.1f us (min %.1f)  mean legal %.0f  sha %s" % (tag, *result), flush=True)
