"""Times the Tron search valued by the caller's network (TronBatch.puct_*: crl_tron_puct_select / _backup, two launches per
simulation for the whole batch, the trees in HBM) and, in the same run and process, the launch floor and the self-contained
territory search beside it.

Per configuration -- P = 4 on 19x19 and on 40x40; --batch trees (4,096) from mid-game positions (N steps of avoid-agent
play with auto-reset from the start layout); seat 0; the avoid model at noise 0.1; S = --simulations (128); the constant
evaluator (equal priors, value 32768: two tensors made once, no launch between select and backup) -- device-event time,
median of --reps after a warm-up:
  * select_us, backup_us: one whole search with an event around every launch, the time of each kind summed over the S
    simulations and divided by S (a launch's share of a growing tree, not the time of a launch on a fixed tree)
  * pair_us: S select + backup pairs back to back between two events, divided by S
  * root_us: puct_root alone
  * puct_ms: the whole puct() -- begin, S pairs, root -- and simulations_per_s = B S / that
  * step_observe_us: TronBatch.step_observe on the same batch, the existing one-launch per-step call, back to back: the
    launch floor; pair_over_two_step_observe = pair_us / (2 step_observe_us)
  * mcts_territory_ms: TronBatch.mcts_territory(S) with the same model, the self-contained search (one flood per leaf, one launch)
  * mean_nodes, mean_depth_last: the node count of a tree, and the edges from the root to the pending leaves of the last
    simulation
Prints one JSON line per configuration and writes them to --out.

    python tools/tron_puct_rate.py [--reps 3] [--batch 4096] [--simulations 128] [--out profiles/tron_puct_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"
SHAPES = [(19, 4), (40, 4)]
AGENT, NOISE = "avoid", 0.1


def _per_kind(tb, S, prior, value, leaves):
    """(select, backup) microseconds per simulation of one search: an event around every launch"""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * S + 1)]
    tb.puct_begin(S, 1, AGENT, NOISE)
    torch.cuda.synchronize()
    ev[0].record()
    for s in range(S):
        tb.puct_select(1.0, 0.5, out=leaves)
        ev[2 * s + 1].record()
        tb.puct_backup(prior, value)
        ev[2 * s + 2].record()
    torch.cuda.synchronize()
    sel = sum(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(S))
    bak = sum(ev[2 * s + 1].elapsed_time(ev[2 * s + 2]) for s in range(S))
    return sel * 1e3 / S, bak * 1e3 / S


def _pairs(tb, S, prior, value, leaves):
    import torch
    tb.puct_begin(S, 1, AGENT, NOISE)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(S):
        tb.puct_select(1.0, 0.5, out=leaves)
        tb.puct_backup(prior, value)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / S


def rows_of(shapes, B, S, reps):
    import torch
    from colosseumrl_amd.batched import TronBatch
    rows = []
    for N, P in shapes:
        tb = TronBatch(N, P, B, device=DEV)
        tb.rollout_avoid(N, seed=7, noise=NOISE)                                  # mid-game positions
        prior = torch.ones((B, 3), dtype=torch.int16, device=DEV)
        value = torch.full((B,), 32768, dtype=torch.int32, device=DEV)

        def evaluate(leaves):
            return prior, value
        root = tb.puct(evaluate, S, 1.0, 0.5, 1, AGENT, NOISE)                    # the warm-up of every launch
        leaves = tb.puct_select(1.0, 0.5)
        kinds = [_per_kind(tb, S, prior, value, leaves) for _ in range(reps + 1)][1:]
        pair = M.median([_pairs(tb, S, prior, value, leaves) for _ in range(reps + 1)][1:])
        live = leaves["pending"] != 0                                           # the last simulation's pending leaves
        last_depth = float(leaves["depth"][live].float().mean()) if bool(live.any()) else None
        root_ms = M.median(M.isolated(lambda: tb.puct_root(out=root), reps, warmup=1))
        puct_ms = M.median(M.isolated(lambda: tb.puct(evaluate, S, 1.0, 0.5, 1, AGENT, NOISE, out=root), reps, warmup=1))
        searched = root["nodes"] > 0
        nodes = float(root["nodes"][searched].float().mean()) if bool(searched.any()) else 0.0
        mo = tb.mcts_territory(S, 1, 1.0, AGENT, NOISE)
        terr_ms = M.median(M.isolated(lambda: tb.mcts_territory(S, 1, 1.0, AGENT, NOISE, out=mo), reps, warmup=1))
        obs = tb.step_observe()
        step_ms = M.median(M.back_to_back(lambda: tb.step_observe(out=obs), S, reps, warmup=S))
        row = {"game": "tron", "N": N, "P": P, "B": B, "S": S, "positions": "%d avoid-agent steps from the start layout" % N,
               "model": "%s, noise %g" % (AGENT, NOISE), "evaluator": "constant (no launch)", "reps": reps,
               "searched_trees": int(searched.sum()),
               "select_us": round(M.median([x[0] for x in kinds]), 2), "backup_us": round(M.median([x[1] for x in kinds]), 2),
               "pair_us": round(pair, 2), "root_us": round(root_ms * 1e3, 2), "puct_ms": round(puct_ms, 4),
               "simulations_per_s": round(B * S / puct_ms * 1e3), "mean_nodes": round(nodes, 1),
               "mean_depth_last": None if last_depth is None else round(last_depth, 2),
               "step_observe_us": round(step_ms * 1e3, 2), "pair_over_two_step_observe": round(pair / (2 * step_ms * 1e3), 3),
               "mcts_territory_ms": round(terr_ms, 4), "puct_over_mcts_territory_time": round(puct_ms / terr_ms, 3)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tron_puct_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 9x9 with four players, 64 trees, 16 simulations")
    args = ap.parse_args()
    M.require_gpu("tron_puct_rate.py")
    import torch
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of([(9, 4)], 64, 16, 1)
    else:
        rows = rows_of(SHAPES, args.batch, args.simulations, args.reps)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
