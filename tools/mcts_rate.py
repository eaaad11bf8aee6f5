"""Times the batched tree search (TTTBatch.mcts: crl_ttt_mcts, one launch, one wave per tree) and, in the same run, flat
Monte Carlo (TTTBatch.flat_mc_action: crl_ttt_playout on every cell plus the pick) with the same number of playouts per
position.

Per configuration -- 3x3 P2, 3x5 K3 P3, 3x3x3 P4, 5x5 K4 P3; --batch positions (4,096), all the empty board (the root of a
game: the longest playouts); S = --simulations (128); R = 16 and 64 -- device-event time of one call, median of --reps after
a warm-up, and from it
  * mcts_ms, simulations_per_s (B S / time)
  * playout_plies_per_s: the plies of the search's random playouts per second.  The kernel does not count plies, so they are
    counted on --sample of the positions by the plain-Python restatement of the contract (tests/mcts_ref.py), whose trees
    must equal the kernel's on those positions bit for bit (the tool stops if they do not), and scaled to the batch
  * flat_mc_ms, flat_mc_playouts: flat_mc_action with ceil(S R / cells) playouts behind every cell, and flat_mc_plies_per_s
    from its own len_sum
Prints one JSON line per configuration and writes them to --out.

    python tools/mcts_rate.py [--reps 3] [--batch 4096] [--simulations 128] [--sample 4] [--out profiles/mcts_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"


def _sampled_plies(dims, k, p, S, R, seed, sample, out):
    """(playouts, plies) per position of the search's random playouts, counted by the restatement on the first `sample`
    positions, whose outputs must be the kernel's"""
    from oracle import oracle as O
    from tests import mcts_ref as M
    st = O.TTTState(dims, k, p, sample)
    count = {"playouts": 0, "plies": 0}
    want = M.ttt_mcts(st, S, R, 256, seed, count=count)
    for key, w in zip(("visits", "value", "nodes", "best"), want):
        if not np.array_equal(out[key][:sample].cpu().numpy().astype(np.int64), w.astype(np.int64)):
            raise SystemExit("mcts_rate.py: %s of the kernel differs from the restatement (%s, S=%d, R=%d)" % (key, dims, S, R))
    return count["playouts"] / sample, count["plies"] / sample


def rows_of(shapes, B, S, Rs, reps, sample, seed=1):
    from colosseumrl_amd.batched import TTTBatch
    rows = []
    for dims, k, p in shapes:
        name = M.shape_name(dims, k, p)
        tb = TTTBatch(dims, k, p, B, device=DEV)
        for R in Rs:
            out = tb.mcts(S, R, seed)
            ms = M.median(M.isolated(lambda: tb.mcts(S, R, seed, out=out), reps, warmup=1))
            playouts, plies = _sampled_plies(dims, k, p, S, R, seed, min(sample, B), out)
            flat_r = -(-S * R // tb.n_cells)
            fo = tb.playout(flat_r, tb._all_cells)
            ms_flat = M.median(M.isolated(lambda: tb.flat_mc_action(flat_r, seed, out=fo), reps, warmup=1))
            flat_plies = int(fo["len_sum"].to(torch.int64).sum())
            row = {"game": "tictactoe", "shape": name, "B": B, "S": S, "R": R, "positions": "empty board",
                   "mcts_ms": round(ms, 4), "simulations_per_s": round(B * S / ms * 1e3),
                   "us_per_simulation_per_wave": round(ms * 1e3 / S, 3),
                   "playouts_per_position": round(playouts, 1), "plies_per_position": round(plies, 1),
                   "playout_plies_per_s": round(plies * B / ms * 1e3), "mean_nodes": round(float(out["nodes"].float().mean()), 1),
                   "flat_mc_playouts_per_position": flat_r * tb.n_cells, "flat_mc_ms": round(ms_flat, 4),
                   "flat_mc_plies_per_s": round(flat_plies / ms_flat * 1e3)}
            row["mcts_over_flat_mc_time"] = round(ms / ms_flat, 3)
            M.emit(row)
            rows.append(row)
        del tb
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--sample", type=int, default=4, help="positions whose playout plies the restatement counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcts_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: one shape, 64 positions, 16 simulations, R = 4")
    args = ap.parse_args()
    M.require_gpu("mcts_rate.py")
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of(M.TTT_SHAPES[:1], 64, 16, [4], 1, 2)
    else:
        rows = rows_of(M.TTT_SHAPES, args.batch, args.simulations, [16, 64], args.reps, args.sample)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
