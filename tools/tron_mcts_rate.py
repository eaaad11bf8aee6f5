"""Times the batched tree search for a seat of Tron (TronBatch.mcts: crl_tron_mcts, one launch, one wave per tree) and, in
the same run, flat Monte Carlo (TronBatch.flat_mc_action: crl_tron_playout on the three first actions plus the pick) with
the same number of playouts per position.

Per configuration -- 19x19 and 40x40, 4 players; --batch positions (4,096) from the middle of avoid-agent games (N steps of
rollout_avoid from the start layout: every game differs, some are a few steps past a restart); seat 0; S = --simulations
(128); R = 16 and 64; the random agent (playouts to their end) and the avoid agent (noise 0.1, playouts capped at 32 steps:
an uncapped avoid playout runs some hundred steps on these boards) as model and in the playouts, which stop with the seat --
device-event time of one call, median of --reps after a warm-up, and from it
  * mcts_ms, simulations_per_s (B S / time), us_per_simulation_per_wave
  * mean_nodes (the kernel's own output), mean_depth and playout_steps_per_s: the kernel counts neither depths nor steps, so
    they are counted on --sample of the positions by the plain-Python restatement of the contract (tests/tron_mcts_ref.py),
    whose trees must equal the kernel's on those positions bit for bit (the tool stops if they do not), and scaled to the
    batch
  * flat_mc_ms: flat_mc_action with ceil(S R / 3) playouts behind every action (the same agent and cap, until="seat_done"), and
    mcts_over_flat_mc_time
Prints one JSON line per configuration and writes them to --out.

    python tools/tron_mcts_rate.py [--reps 3] [--batch 4096] [--simulations 128] [--sample 2] [--out profiles/tron_mcts_rate.jsonl] [--tiny]
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
NOISE = 0.1
CAP = {"random": 0, "avoid": 32}                           # max_steps of the playouts, per agent


def _sampled(tb, S, R, agent, seed, sample, out):
    """(mean leaf depth, playouts, playout steps, closed leaves) per position, counted by the restatement on the first
    `sample` positions, whose outputs must be the kernel's"""
    from oracle import oracle as O
    from tests import tron_mcts_ref as T
    st = O.TronState(tb.N, tb.P, sample)
    st.board[:] = tb.board[:sample].cpu().numpy()
    for name, t in (("heads", tb.heads), ("dirs", tb.dirs), ("deaths", tb.deaths)):
        getattr(st, name)[:] = t[:, :sample].cpu().numpy()
    tc = tb.tcount[:sample].cpu().numpy().view(np.uint32)
    count = T.new_count()
    want = T.tron_mcts(st, S, R, 256, seed, tb.first_env_id, tc, None, agent, NOISE, CAP[agent], count)
    for key, w in zip(("visits", "value", "nodes", "best"), want):
        if not np.array_equal(out[key][:sample].cpu().numpy().astype(np.int64), w.astype(np.int64)):
            raise SystemExit("tron_mcts_rate.py: %s of the kernel differs from the restatement (N=%d, S=%d, R=%d, %s)"
                             % (key, tb.N, S, R, agent))
    played = max(1, int((want[2] > 0).sum()))
    return count["depth"] / (played * S), count["playouts"] / sample, count["steps"] / sample, count["closed"] / sample


def rows_of(sizes, B, S, Rs, reps, sample, seed=1):
    from colosseumrl_amd.batched import TronBatch
    rows = []
    for N in sizes:
        tb = TronBatch(N, 4, B, device=DEV)
        tb.rollout_avoid(N, 3, NOISE)                            # mid-game positions
        for agent in ("random", "avoid"):
            for R in Rs:
                out = tb.mcts(S, R, seed, 1.0, agent, NOISE, None, CAP[agent])
                ms = M.median(M.isolated(lambda: tb.mcts(S, R, seed, 1.0, agent, NOISE, None, CAP[agent], out), reps, warmup=1))
                depth, playouts, steps, closed = _sampled(tb, S, R, agent, seed, min(sample, B), out)
                flat_r = -(-S * R // 3)
                fo = tb.playout(flat_r, tb._moves3, seed, agent, NOISE, None, "seat_done", CAP[agent])
                ms_flat = M.median(M.isolated(lambda: tb.flat_mc_action(flat_r, seed, agent, NOISE, None, "seat_done", CAP[agent], fo),
                                              reps, warmup=1))
                nodes = out["nodes"].float()
                row = {"game": "tron", "N": N, "P": 4, "B": B, "S": S, "R": R, "agent": agent, "noise": NOISE, "max_steps": CAP[agent],
                       "positions": "%d avoid-agent steps from the start layout" % N,
                       "mcts_ms": round(ms, 4), "simulations_per_s": round(B * S / ms * 1e3),
                       "us_per_simulation_per_wave": round(ms * 1e3 / S, 3),
                       "mean_nodes": round(float(nodes[nodes > 0].mean()), 1), "mean_depth": round(depth, 2),
                       "playouts_per_position": round(playouts, 1), "closed_leaves_per_position": round(closed, 1),
                       "playout_steps_per_position": round(steps, 1), "playout_steps_per_s": round(steps * B / ms * 1e3),
                       "flat_mc_playouts_per_position": 3 * flat_r, "flat_mc_ms": round(ms_flat, 4),
                       "flat_mc_steps_per_s": round(int(fo["len_sum"].to(torch.int64).sum()) / ms_flat * 1e3)}
                row["mcts_over_flat_mc_time"] = round(ms / ms_flat, 3)
                M.emit(row)
                rows.append(row)
        del tb
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--sample", type=int, default=2, help="positions whose depths and playout steps the restatement counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tron_mcts_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 9x9, 64 positions, 16 simulations, R = 4")
    args = ap.parse_args()
    M.require_gpu("tron_mcts_rate.py")
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of([9], 64, 16, [4], 1, 2)
    else:
        rows = rows_of([19, 40], args.batch, args.simulations, [16, 64], args.reps, args.sample)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
