"""Times the Blokus tree search with progressive widening (BlokusBatch.mcts: crl_blokus_mcts, one launch) and, in the same
run, flat Monte Carlo (BlokusBatch.flat_mc_action: crl_blokus_playout on drawn candidates plus the pick) with the same number
of playouts per position.

--batch positions (1,024), each a game after --plies (32) plies of the random agent, made by the CPU oracle; S =
--simulations (128); W = --width (8); R = 1 (one wave per tree) and 16 (one workgroup per tree) -- device-event time of one
call, median of --reps after a warm-up, and from it
  * mcts_ms, simulations_per_s (B S / time)
  * playout_plies_per_s: the plies of the search's random playouts per second.  The kernel does not count plies, so they are
    counted on --sample of the positions by the plain-Python restatement of the contract (tests/blokus_mcts_ref.py), whose
    trees must equal the kernel's on those positions bit for bit (the tool stops if they do not), and scaled to the batch
  * flat_mc_ms: flat_mc_action over W uniformly drawn legal candidates with S R / W playouts behind each, and
    flat_mc_plies_per_s from its own len_sum
Prints one JSON line per R and writes them to --out.

    python tools/blokus_mcts_rate.py [--reps 3] [--batch 1024] [--simulations 128] [--width 8] [--plies 32] [--sample 1]
                                     [--out profiles/blokus_mcts_rate.jsonl] [--tiny]
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
SEED, FIRST_ENV_ID = 1, 7000


def _sampled_plies(st, S, R, W, sample, out):
    """(playouts, plies) per position of the search's random playouts, counted by the restatement on the first `sample`
    positions, whose outputs must be the kernel's"""
    from tests import blokus_mcts_ref as ref
    from tests.blokus_ref import blokus_one
    count = {"playouts": 0, "plies": 0}
    for b in range(sample):
        want = ref.search(blokus_one(st, b), S, R, W, 256, SEED, FIRST_ENV_ID + b, 0, None, count)
        have = tuple(out[k][b].cpu().tolist() for k in ("ids", "visits", "value", "nodes", "best"))
        if have != tuple(want):
            raise SystemExit("blokus_mcts_rate.py: the kernel's tree differs from the restatement's (position %d, S=%d, R=%d, W=%d):\n"
                             "%s\n%s" % (b, S, R, W, have, want))
    return count["playouts"] / sample, count["plies"] / sample


def rows_of(B, S, W, Rs, plies, reps, sample):
    from oracle import oracle as O
    from tests.gpu_util import blokus_batch
    st = O.BlokusState(B)
    O.blokus_rollout(st, SEED + 1, FIRST_ENV_ID, plies, n_threads=min(16, os.cpu_count() or 1))
    if st.n_episodes.any():
        raise SystemExit("blokus_mcts_rate.py: a game ended within %d plies" % plies)
    st.tcount[:] = 0
    bb = blokus_batch(st, FIRST_ENV_ID)
    count = bb.valid()
    rank = (torch.rand((B, W), device=DEV, generator=torch.Generator(DEV).manual_seed(3)) * count.clamp(min=1)[:, None]).to(torch.int32)
    cand = torch.stack([bb.select(rank[:, a].contiguous())[0] for a in range(W)], dim=1).contiguous()
    rows = []
    for R in Rs:
        out = bb.mcts(S, R, None, W, SEED)
        ms = M.median(M.isolated(lambda: bb.mcts(S, R, None, W, SEED, out=out), reps, warmup=1))
        playouts, n_plies = _sampled_plies(st, S, R, W, min(sample, B), out)
        flat_r = max(1, S * R // W)
        fo = bb.playout(flat_r, cand, SEED)
        ms_flat = M.median(M.isolated(lambda: bb.flat_mc_action(cand, flat_r, SEED, out=fo), reps, warmup=1))
        flat_plies = int(fo["len_sum"].to(torch.int64).sum())
        row = {"game": "blokus", "B": B, "S": S, "W": W, "R": R, "positions": "after %d random plies" % plies,
               "mapping": "workgroup per tree" if R >= 4 else "wave per tree",
               "mcts_ms": round(ms, 4), "simulations_per_s": round(B * S / ms * 1e3),
               "playouts_per_position": round(playouts, 1), "plies_per_position": round(n_plies, 1),
               "playout_plies_per_s": round(n_plies * B / ms * 1e3), "mean_nodes": round(float(out["nodes"].float().mean()), 1),
               "flat_mc_candidates": W, "flat_mc_playouts_per_position": flat_r * W, "flat_mc_ms": round(ms_flat, 4),
               "flat_mc_plies_per_s": round(flat_plies / ms_flat * 1e3), "mcts_over_flat_mc_time": round(ms / ms_flat, 3)}
        M.emit(row)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--plies", type=int, default=32, help="random plies from the fresh position to each timed position")
    ap.add_argument("--sample", type=int, default=1, help="positions whose trees the restatement rebuilds and whose plies it counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blokus_mcts_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 32 positions after 48 plies, 8 simulations, W = 4, R = 1 and 4")
    args = ap.parse_args()
    M.require_gpu("blokus_mcts_rate.py")
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of(32, 8, 4, [1, 4], 48, 1, 1)
    else:
        rows = rows_of(args.batch, args.simulations, args.width, [1, 16], args.plies, args.reps, args.sample)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
