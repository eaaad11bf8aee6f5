"""Times one learner step against the random agent (step_single) for TicTacToe and Blokus against the launch chain it replaces.

For each game, at B games (Blokus 16,384, TicTacToe 262,144), device-event time per learner step of
  * fused  -- TTTBatch / BlokusBatch.step_single (crl_*_step_single, ONE launch: the learner's ply and the P - 1 opponents')
  * chain  -- step_observe(learner action) + (P - 1) x step_observe(None): the same launch count without the per-game seat
              logic (so NOT a correct single-player step once games end at different plies: a speed baseline only)
  * ply    -- the random-agent rollout (crl_*_rollout) per ply, times P plies = the rollout's price of one learner step
after a warm-up of each.  The learner's actions are drawn beforehand, a fresh one per step: TicTacToe a uniform cell
(an occupied one passes) in both; Blokus a uniform rank in [0, 64) into its legal list (CRL_STEP_RANK_ACTION; a rank past
the list passes) in the fused call, the random agent's draw (step_observe(None): the same count + select) in the chain.
Prints one JSON line per game and writes them all to --out.

    python tools/single_rate.py [--blokus-batch 16384] [--ttt-batch 262144] [--steps 20] [--reps 5] [--out FILE]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402


def _min_median_us(fn, reps):
    ts = [ms * 1e3 for ms in M.isolated(fn, reps)]
    return min(ts), M.median(ts)


def _measure(name, B, P, make, steps, reps, fused_action, chain_action, rank=False, seed=3):
    """fused_action(k) / chain_action(k): the learner's action of timed step k (precomputed, so no launch of its own)."""
    single, chain, roll = make(), make(), make()
    seat = torch.zeros((B,), dtype=torch.int8, device="cuda:0")
    single.step_single(seat, None, seed)
    outs = {}

    def run_single():
        for k in range(steps):
            outs["s"] = single.step_single(seat, fused_action(k), seed, out=outs.get("s"), **({"rank": True} if rank else {}))

    def run_chain():
        for k in range(steps):
            outs["c"] = chain.step_observe(chain_action(k), seed, out=outs.get("c"))
            for _ in range(P - 1):
                outs["c"] = chain.step_observe(None, seed, out=outs.get("c"))

    run_single()
    run_chain()
    roll.rollout(steps * P, seed)
    t_single = _min_median_us(run_single, reps)
    t_chain = _min_median_us(run_chain, reps)
    t_roll = _min_median_us(lambda: roll.rollout(steps * P, seed), reps)
    torch.cuda.synchronize()
    row = {"game": name, "B": B, "P": P, "steps": steps,
           "fused_us_per_step": round(t_single[1] / steps, 2), "chain_us_per_step": round(t_chain[1] / steps, 2),
           "rollout_us_per_ply": round(t_roll[1] / (steps * P), 2),
           "rollout_us_per_learner_step": round(t_roll[1] / steps, 2),
           "fused_us_per_step_min": round(t_single[0] / steps, 2), "chain_us_per_step_min": round(t_chain[0] / steps, 2),
           "chain_over_fused": round(t_chain[1] / t_single[1], 2),
           "fused_over_rollout": round(t_single[1] / t_roll[1], 2),
           "fused_done_per_game_step": round(float(outs["s"]["done"].float().mean()), 4)}
    M.emit(row)
    del single, chain, roll
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blokus-batch", type=int, default=16384)
    ap.add_argument("--ttt-batch", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from colosseumrl_amd.batched import BlokusBatch, TTTBatch
    M.require_gpu("single_rate.py")
    torch.cuda.set_device(0)
    rows = []
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    for dims, k, p in (((3, 3), 3, 2), ((3, 5), 3, 3), ((3, 3, 3), 3, 4)):
        name = "ttt_%s_k%d_p%d" % ("x".join(map(str, dims)), k, p)
        cells = 1
        for d in dims:
            cells *= d
        acts = [torch.randint(0, cells, (args.ttt_batch,), generator=gen, device="cuda:0") for _ in range(args.steps)]
        acts8 = [a.to(torch.int8) for a in acts]
        rows.append(_measure(name, args.ttt_batch, p, lambda: TTTBatch(dims, k, p, args.ttt_batch, device="cuda:0"),
                             args.steps, args.reps, lambda i: acts[i], lambda i: acts8[i]))
    ranks = [torch.randint(0, 64, (args.blokus_batch,), generator=gen, device="cuda:0") for _ in range(args.steps)]
    rows.append(_measure("blokus", args.blokus_batch, 4, lambda: BlokusBatch(args.blokus_batch, device="cuda:0"),
                         args.steps, args.reps, lambda i: ranks[i], lambda i: None, rank=True))
    if args.out:
        M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
