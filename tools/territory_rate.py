"""Times the Voronoi territory call (TronBatch.territory: crl_tron_territory, one launch) and the territory-greedy agent
(TronBatch.sample_territory) next to the calls they stand beside.

Positions are mid-game ones (rollout_avoid, noise 0.1, N steps from the start layout; P = 4).  Per shape -- 4,096 positions x
3 candidates on 19x19 and 40x40, and 65,536 positions with no candidate on 20x20 -- device-event times, median of --reps
after a warm-up:
  * ms, instances_per_s of the territory call, and mean_depth, the mean number of flood levels that claimed a cell (from a
    numpy flood of the first --depth-sample instances);
  * observe_all_ms: crl_tron_observe_all on the same boards, a pass over the same bytes;
  * with candidates: decision_ms, the whole territory_action (territory + arg-max), and flat_mc_ms, flat_mc_action with 32
    avoid playouts per move, the evaluator this one is the cheap alternative to; decision_cheaper says which is faster;
  * sample_territory_ms beside sample_avoid_ms: the two scripted agents for all four players.
Prints one JSON line per shape and writes them to --out.

    python tools/territory_rate.py [--reps 3] [--out profiles/territory_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"


def _mean_depth(tb, n):
    """mean number of levels that claim a cell, over the first n positions with nobody forced (the numpy flood of the tests)"""
    from tests import territory_ref as R
    n = min(n, tb.B)
    board = tb.board[:n].cpu().numpy().reshape(n, -1)
    heads, dirs, deaths = (x[:, :n].cpu().numpy() for x in (tb.heads, tb.dirs, tb.deaths))
    free, first, _ = R.first_cells(tb.N, board, heads, dirs, deaths)
    return float(R.areas_by_levels(free, first)[1].mean())


def rows(shapes, reps, playouts, depth_sample):
    import torch
    from colosseumrl_amd.batched import TronBatch
    out = []
    for N, B, A in shapes:
        tb = TronBatch(N, 4, B, device=DEV)
        tb.rollout_avoid(N, 7, 0.1)
        torch.cuda.synchronize()
        cand = torch.arange(3, dtype=torch.int32, device=DEV).expand(B, 3).contiguous() if A == 3 else None
        to = tb.territory(cand)
        ms = M.median(M.isolated(lambda: tb.territory(cand, out=to), reps, warmup=1))
        ob = tb.observe_all()
        oms = M.median(M.isolated(lambda: tb.observe_all(out=ob), reps, warmup=1))
        acts = torch.zeros((4, B), dtype=torch.int8, device=DEV)
        tms = M.median(M.isolated(lambda: tb.sample_territory(3, 0.1, out=acts, advance=False), reps, warmup=1))
        ams = M.median(M.isolated(lambda: tb.sample_avoid(3, 0.1, out=acts, advance=False), reps, warmup=1))
        row = {"N": N, "P": 4, "B": B, "A": A, "ms": round(ms, 4), "instances_per_s": B * A / (ms * 1e-3),
               "mean_depth": round(_mean_depth(tb, depth_sample), 2), "observe_all_ms": round(oms, 4),
               "sample_territory_ms": round(tms, 4), "sample_avoid_ms": round(ams, 4)}
        if A == 3:
            dms = M.median(M.isolated(lambda: tb.territory_action(out=to), reps, warmup=1))
            po = tb.playout(playouts, cand, 1, agent="avoid", until="seat_done")
            fms = M.median(M.isolated(lambda: tb.flat_mc_action(playouts, 1, "avoid", 0.1, None, "seat_done", 0, po), reps, warmup=1))
            row.update({"decision_ms": round(dms, 4), "flat_mc_playouts": playouts, "flat_mc_ms": round(fms, 4),
                        "decision_cheaper": dms < fms, "flat_mc_over_decision": fms / dms})
        M.emit(row)
        out.append(row)
        del tb
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--playouts", type=int, default=32)
    ap.add_argument("--depth-sample", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "territory_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a seconds-long smoke run (64 positions, 19x19 x 3 and 20x20 x 1, 4 playouts)")
    a = ap.parse_args()
    M.require_gpu("territory_rate.py")
    if a.tiny:
        res = rows([(19, 64, 3), (20, 64, 1)], 1, 4, 16)
    else:
        res = rows([(19, 4096, 3), (40, 4096, 3), (20, 65536, 1)], a.reps, a.playouts, a.depth_sample)
    M.write_rows(a.out, res)


if __name__ == "__main__":
    main()
