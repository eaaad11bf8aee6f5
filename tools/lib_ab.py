#!/usr/bin/env python3
"""A/B of library VARIANTS (tools/lib_variant.sh) on one device: every variant runs in its own process (the library is
loaded once per process), rounds interleaved so that clock drift hits all alike.

    python tools/lib_ab.py [--isolated] [--rounds 3] <workload> <steps per launch>[,<steps>...] <tag>=<path to .so> [<tag>=<path> ...]

Default: launches back to back (steady state).  --isolated: one launch between two synchronisations, the way bench.py's
contract region times a short launch (HIP-event time of the launch and wall clock of launch + events + synchronise).

workload: a bench.py WORKLOADS name.  Prints per variant and launch length the median / min kernel time over the rounds
(HIP events around a batch of launches) and env-steps/s."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402


def child(wl, Ts, isolated):
    """one round of one variant: {T: [median ms, min ms]}, isolated {T: [median ms, 5th percentile ms, median wall ms]}, as a
    JSON line behind "AB " """
    import torch
    import bench
    game, kw, batch, chunk = bench.WORKLOADS[wl][:4]
    st = bench.make_stepper(game, kw, batch, torch.device("cuda", 0), 0)
    out = {}
    for T in Ts:
        if isolated:
            ev, wall = M.isolated(lambda: st.rollout(T, 0), 300, warmup=20, wall=True)
            out[str(T)] = [M.median(ev), sorted(ev)[15], M.median(wall)]
        else:
            calls = max(3, min(200, int(0.05 / max(1e-5, T * 4e-7))))
            ts = M.back_to_back(lambda: st.rollout(T, 0), calls, rounds=5, warmup=3)
            out[str(T)] = [M.median(ts), min(ts)]
    print("AB " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--isolated", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("workload")
    ap.add_argument("steps")
    ap.add_argument("variants", nargs="*", metavar="tag=path")
    a = ap.parse_args()
    wl, Ts = a.workload, [int(t) for t in a.steps.split(",")]
    if a.child:
        return child(wl, Ts, a.isolated)
    variants = [v.split("=", 1) for v in a.variants]
    import bench
    batch = bench.WORKLOADS[wl][2]
    cmd = [sys.executable, os.path.abspath(__file__), "--child", wl, a.steps] + (["--isolated"] if a.isolated else [])
    res = {tag: {str(T): [] for T in Ts} for tag, _ in variants}
    for tag, result in M.alternate(cmd, variants, a.rounds, 600, "AB "):
        for T, v in result.items():
            res[tag][T].append(v)
    for T in Ts:
        for tag, _ in variants:
            med = M.median([v[0] for v in res[tag][str(T)]])
            mn = min(v[1] for v in res[tag][str(T)])
            if a.isolated:
                wall = M.median([v[2] for v in res[tag][str(T)]])
                print("%s T=%-5d %-12s isolated launch: events median %7.2f us  p5 %7.2f us   launch+2 events+sync wall %7.2f us" % (wl, T, tag, med * 1e3, mn * 1e3, wall * 1e3), flush=True)
                continue
            print("%s T=%-5d %-12s median %9.4f ms  min %9.4f ms  -> %.4g env-steps/s" % (wl, T, tag, med, mn, batch * T / (med * 1e-3)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
