"""Times the Tron tree search with Voronoi territory at the leaves (TronBatch.mcts_territory: crl_tron_mcts_territory, one
launch, one wave per tree, one flood per leaf) and, in the same run and on the same positions, what it is to be compared
with: the playout search (TronBatch.mcts) at R = 16 and R = 64 with the same S and model agent, and the one-ply
territory-greedy pick (TronBatch.territory_action).

Per configuration -- 19x19 and 40x40, 4 players; --batch positions (4,096) from the middle of avoid-agent games (N steps of
rollout_avoid from the start layout); seat 0; S = --simulations (128); the random and the avoid agent (noise 0.1) as the model
of the tree steps; the playout search's playouts as tools/tron_mcts_rate.py runs them (random to their end, avoid capped at
32 steps) -- device-event time of one call, median of --reps after a warm-up, and from it
  * mcts_territory_ms, simulations_per_s (B S / time), us_per_simulation_per_wave
  * mcts_r16_ms, mcts_r64_ms, territory_action_ms and the ratios territory_over_mcts_r16_time / _r64_time /
    territory_over_territory_action_time
  * mean_nodes (the kernel's own output); mean_depth, closed_leaves_per_position and flood_levels_per_leaf: the kernel counts
    none of them, so they are counted on --sample of the positions by the plain-Python restatement of the contract
    (tests/tron_mcts_territory_ref.py), whose trees must equal the kernel's on those positions bit for bit (the tool stops if
    they do not)
Prints one JSON line per configuration and writes them to --out.

    python tools/tron_mcts_territory_rate.py [--reps 3] [--batch 4096] [--simulations 128] [--sample 2]
                                             [--out profiles/tron_mcts_territory_rate.jsonl] [--tiny]
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
VALUE_SCALE = 256
CAP = {"random": 0, "avoid": 32}                           # max_steps of the playout search's playouts, per agent


def _sampled(tb, S, agent, seed, sample, out):
    """(mean leaf depth, closed leaves per position, flood levels per flooded leaf), counted by the restatement on the first
    `sample` positions, whose outputs must be the kernel's"""
    from oracle import oracle as O
    from tests import tron_mcts_territory_ref as T
    st = O.TronState(tb.N, tb.P, sample)
    st.board[:] = tb.board[:sample].cpu().numpy()
    for name, t in (("heads", tb.heads), ("dirs", tb.dirs), ("deaths", tb.deaths)):
        getattr(st, name)[:] = t[:, :sample].cpu().numpy()
    tc = tb.tcount[:sample].cpu().numpy().view(np.uint32)
    count = T.new_count()
    want = T.tron_mcts_territory(st, S, VALUE_SCALE, 256, seed, tb.first_env_id, tc, None, agent, NOISE, count, "bits")
    for key, w in zip(("visits", "value", "nodes", "best"), want):
        if not np.array_equal(out[key][:sample].cpu().numpy().astype(np.int64), w.astype(np.int64)):
            raise SystemExit("tron_mcts_territory_rate.py: %s of the kernel differs from the restatement (N=%d, S=%d, %s)"
                             % (key, tb.N, S, agent))
    played = max(1, int((want[2] > 0).sum()))
    return count["depth"] / (played * S), count["closed"] / sample, count["levels"] / max(1, count["flooded"])


def rows_of(sizes, B, S, reps, sample, seed=1):
    from colosseumrl_amd.batched import TronBatch
    rows = []
    for N in sizes:
        tb = TronBatch(N, 4, B, device=DEV)
        tb.rollout_avoid(N, 3, NOISE)                            # mid-game positions
        to = tb.territory(tb._moves3)
        ms_greedy = M.median(M.isolated(lambda: tb.territory_action(None, to), reps, warmup=1))
        for agent in ("random", "avoid"):
            out = tb.mcts_territory(S, seed, 1.0, agent, NOISE, None, VALUE_SCALE)
            ms = M.median(M.isolated(lambda: tb.mcts_territory(S, seed, 1.0, agent, NOISE, None, VALUE_SCALE, out), reps, warmup=1))
            depth, closed, levels = _sampled(tb, S, agent, seed, min(sample, B), out)
            nodes = out["nodes"].float()
            row = {"game": "tron", "N": N, "P": 4, "B": B, "S": S, "agent": agent, "noise": NOISE, "value_scale": VALUE_SCALE,
                   "positions": "%d avoid-agent steps from the start layout" % N,
                   "mcts_territory_ms": round(ms, 4), "simulations_per_s": round(B * S / ms * 1e3),
                   "us_per_simulation_per_wave": round(ms * 1e3 / S, 3),
                   "mean_nodes": round(float(nodes[nodes > 0].mean()), 1), "mean_depth": round(depth, 2),
                   "closed_leaves_per_position": round(closed, 1), "flood_levels_per_leaf": round(levels, 1)}
            for R in (16, 64):
                po = tb.mcts(S, R, seed, 1.0, agent, NOISE, None, CAP[agent])
                ms_r = M.median(M.isolated(lambda: tb.mcts(S, R, seed, 1.0, agent, NOISE, None, CAP[agent], po), reps, warmup=1))
                row["mcts_r%d_ms" % R] = round(ms_r, 4)
                row["territory_over_mcts_r%d_time" % R] = round(ms / ms_r, 3)
            row["mcts_max_steps"] = CAP[agent]
            row["territory_action_ms"] = round(ms_greedy, 4)
            row["territory_over_territory_action_time"] = round(ms / ms_greedy, 3)
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
    ap.add_argument("--sample", type=int, default=2, help="positions whose depths and flood levels the restatement counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tron_mcts_territory_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 9x9, 64 positions, 16 simulations")
    args = ap.parse_args()
    M.require_gpu("tron_mcts_territory_rate.py")
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of([9], 64, 16, 1, 2)
    else:
        rows = rows_of([19, 40], args.batch, args.simulations, args.reps, args.sample)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
