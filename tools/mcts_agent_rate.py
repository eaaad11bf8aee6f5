"""Times the tree search as a seated agent: one learner step against search opponents (TTTBatch.step_single(opponent="mcts"):
crl_ttt_step_single_mcts, one launch, one wave per game) and self-play of the search (TTTBatch.rollout_mcts), and in the same
process the floor of any composition of that step from the calls there were before: (P - 1) x TTTBatch.mcts plus one
step_single against the random agent.

Per configuration -- 3x3 P2, 3x5 K3 P3, 3x3x3 P4, 5x5 K4 P3; --batch games (4,096) with the learner at seat 0, a uniformly
random learner; S = --simulations (128), R = --playouts (16), noise 0 -- device-event times, median of --reps after a warm-up:
  * step_single_mcts_ms: one step_single(opponent="mcts") call, and searches_per_call: the opponents' plies of a call per
    game, from tcount (at noise 0 every opponent ply searches), and ms_per_search: the call's time over the searches a game
    plays in it
  * mcts_ms (one TTTBatch.mcts call on the same positions), step_single_random_ms, floor_ms = (P - 1) mcts_ms +
    step_single_random_ms and step_over_floor = step_single_mcts_ms / floor_ms
  * rollout_mcts_ms for --plies (8) plies and rollout_plies_per_s
Prints one JSON line per configuration and writes them to --out.

    python tools/mcts_agent_rate.py [--reps 3] [--batch 4096] [--simulations 128] [--playouts 16] [--plies 8]
                                    [--out profiles/mcts_agent_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"


def _uniform_actions(valid, cells, gen):
    """int64 [B]: a uniformly random empty cell of every game (valid: the empties masks)"""
    bits = 1 << torch.arange(cells, device=valid.device, dtype=torch.int64)
    free = (valid.to(torch.int64)[:, None] & bits[None, :]) != 0
    return torch.rand(free.shape, generator=gen, device=valid.device).masked_fill(~free, -1.0).argmax(dim=1).to(torch.int64)


def _steps(tb, seat, gen, reps, seed, timed=None, **opponent):
    """reps + 1 learner steps (the first a warm-up) of a uniformly random learner: (median ms, opponents' plies per game and
    call).  timed(): also runs after every step but the warm-up; its times come back as a third value"""
    out = tb.step_single(seat, None, seed, **opponent)
    ts, extra, plies = [], [], 0
    for i in range(reps + 1):
        act = _uniform_actions(out["valid"], tb.n_cells, gen)
        before = tb.tcount.clone()
        ms = M.isolated(lambda: tb.step_single(seat, act, seed, out=out, **opponent), 1)[0]
        if i:
            ts.append(ms)
            plies += int((tb.tcount - before).to(torch.int64).sum()) - tb.B      # (the learner's ply is one of them)
            if timed is not None:
                extra += M.isolated(timed, 1)
    return M.median(ts), plies / (reps * tb.B), extra


def rows_of(shapes, B, S, R, T, reps, seed=1):
    from colosseumrl_amd.batched import TTTBatch
    rows = []
    for dims, k, p in shapes:
        name = M.shape_name(dims, k, p)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(7)
        seat = torch.zeros(B, dtype=torch.int8, device=DEV)
        tb = TTTBatch(dims, k, p, B, device=DEV)
        search = tb.mcts(S, R, seed)
        ms, searches, mcts_ts = _steps(tb, seat, gen, reps, seed, timed=lambda: tb.mcts(S, R, seed, out=search),
                                       opponent="mcts", noise=0.0, simulations=S, playouts=R)
        tr = TTTBatch(dims, k, p, B, device=DEV)
        ms_random, _, _ = _steps(tr, seat, gen, reps, seed)
        tb.reset()
        ms_roll = M.median(M.isolated(lambda: tb.rollout_mcts(T, S, R, seed), reps, warmup=1))
        ms_mcts = M.median(mcts_ts)
        floor = (p - 1) * ms_mcts + ms_random
        row = {"game": "tictactoe", "shape": name, "B": B, "S": S, "R": R, "noise": 0.0, "learner": "uniform, seat 0",
               "step_single_mcts_ms": round(ms, 4), "searches_per_call": round(searches, 3),
               "ms_per_search": round(ms / max(searches, 1e-9), 4), "mcts_ms": round(ms_mcts, 4),
               "step_single_random_ms": round(ms_random, 4), "floor_ms": round(floor, 4), "step_over_floor": round(ms / floor, 3),
               "rollout_plies": T, "rollout_mcts_ms": round(ms_roll, 4), "rollout_plies_per_s": round(B * T / ms_roll * 1e3)}
        M.emit(row)
        rows.append(row)
        del tb, tr
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--playouts", type=int, default=16)
    ap.add_argument("--plies", type=int, default=8, help="plies of a rollout_mcts launch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcts_agent_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: one shape, 64 games, 16 simulations, R = 4, 2 plies")
    args = ap.parse_args()
    M.require_gpu("mcts_agent_rate.py")
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of(M.TTT_SHAPES[:1], 64, 16, 4, 2, 1)
    else:
        rows = rows_of(M.TTT_SHAPES, args.batch, args.simulations, args.playouts, args.plies, args.reps)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
