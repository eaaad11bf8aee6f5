"""Times the Blokus tree search as a seated agent (crl_blokus_sample_mcts / crl_blokus_step_single_mcts /
crl_blokus_rollout_mcts, each one launch) beside what it is made of, all in one process.

--batch positions (1,024), each a game after --plies (32) plies of the random agent, made by the CPU oracle; S =
--simulations (128); W = --width (8); R = 1 (one wave per game) and 16 (one workgroup per game); noise 0 -- device-event time
of one call from the same positions (the state is put back before every call), median and [min, max] of --reps after a warm-up:
  * sample_ms: BlokusBatch.sample_mcts beside mcts_ms: BlokusBatch.mcts on the same positions (the agent's move IS that
    search's best: the tool stops unless every row agrees)
  * step_ms: BlokusBatch.step_single(opponent="mcts") with a uniformly random learner (by rank) at the seat to move, beside
    floor_ms = 3 x mcts_ms + step_random_ms (step_single against the random agent): what three masked searches and the
    plain step cost at the least when composed from separate calls; opponent_plies_per_game: the plies the opponents played
    per game in the call (each a search where the mover has an action; three unless a game ended and restarted)
  * rollout_ms: BlokusBatch.rollout_mcts of --rollout-plies (8) plies, and rollout_plies_per_s = B plies / time
The first --sample games are replayed by the plain-Python restatement of the contract (tests/blokus_mcts_agent_ref.py): the
tool stops unless it reproduces their sampled actions and, for the step, their opponents' plies, state and counters.
Prints one JSON line per R and writes them to --out.

    python tools/blokus_mcts_agent_rate.py [--reps 3] [--batch 1024] [--simulations 128] [--width 8] [--plies 32]
                                           [--rollout-plies 8] [--sample 1] [--out profiles/blokus_mcts_agent_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"
SEED, FIRST_ENV_ID = 1, 7000
STATE = ("occ", "inv", "score", "round", "to_move", "tcount", "tstep")
TOOL = "blokus_mcts_agent_rate.py"


def _timed(restore, fn, reps):
    """median, [min, max] of `fn` from the restored state, after one warm-up call"""
    restore()
    fn()
    ms = []
    for _ in range(reps):
        restore()
        ms.append(M.isolated(fn, 1)[0])
    return M.spread(ms)


def _check_sample(st, act, S, R, W, sample):
    """the restatement's move for the first `sample` games is the kernel's"""
    from tests import blokus_mcts_agent_ref as ref
    from tests.blokus_ref import blokus_one
    for b in range(sample):
        want = ref.agent_action(blokus_one(st, b), 0, FIRST_ENV_ID + b, SEED, W, S, R, 256, 0.0)
        if int(act[b]) != want:
            raise SystemExit("%s: sample_mcts differs from the restatement (game %d, S=%d, R=%d, W=%d): %d, %d"
                             % (TOOL, b, S, R, W, int(act[b]), want))


def _check_step(st, seat, ranks, bb, S, R, W, sample):
    """the restatement's step of the first `sample` games leaves the kernel's state and counters -> searches per game there"""
    from tests import blokus_mcts_agent_ref as ref
    from tests import blokus_positions as BP
    one = BP.clone(st, list(range(sample)))
    log = []
    ref.step_single_mcts(one, seat[:sample], ranks[:sample], SEED, W, S, R, 256, 0.0, first_env_id=FIRST_ENV_ID, rank=True, log=log)
    for k in ("occ", "inv", "score", "round", "to_move", "tcount"):
        have = getattr(bb, k)[:sample].cpu().numpy().view(np.uint32)
        if not np.array_equal(have, getattr(one, k).view(np.uint32)):
            raise SystemExit("%s: step_single(opponent='mcts') differs from the restatement in %s (S=%d, R=%d, W=%d)" % (TOOL, k, S, R, W))
    return sum(1 for e in log if e[2] == "searched") / sample


def rows_of(B, S, W, Rs, plies, reps, sample, rollout_plies):
    import torch
    from oracle import oracle as O
    from tests.gpu_util import blokus_batch
    st = O.BlokusState(B)
    O.blokus_rollout(st, SEED + 1, FIRST_ENV_ID, plies, n_threads=min(16, os.cpu_count() or 1))
    if st.n_episodes.any():
        raise SystemExit("%s: a game ended within %d plies" % (TOOL, plies))
    st.tcount[:] = 0
    st.tstep[:] = 0
    bb = blokus_batch(st, FIRST_ENV_ID)
    keep = {k: getattr(bb, k).clone() for k in STATE}

    def restore():
        for k, v in keep.items():
            getattr(bb, k).copy_(v)
    seat_np = (st.to_move & 3).astype(np.int8)                   # the learner is the player to move
    seat = torch.from_numpy(seat_np).to(DEV)
    n_valid = bb.valid()
    u = torch.rand((B,), device=DEV, dtype=torch.float64, generator=torch.Generator(DEV).manual_seed(3))
    ranks = torch.minimum((u * n_valid).to(torch.int64), (n_valid - 1).clamp(min=0).to(torch.int64))
    ranks_np = ranks.cpu().numpy()
    out_r = bb.step_single(seat, ranks, SEED, rank=True)
    ms_random, _ = _timed(restore, lambda: bb.step_single(seat, ranks, SEED, rank=True, out=out_r), reps)
    rows = []
    for R in Rs:
        search = dict(simulations=S, playouts=R, width=W, exploration=1.0, noise=0.0)
        restore()
        tree = bb.mcts(S, R, None, W, SEED)
        ms_mcts, mcts_range = _timed(restore, lambda: bb.mcts(S, R, None, W, SEED, out=tree), reps)
        ms_sample, sample_range = _timed(restore, lambda: bb.sample_mcts(seed=SEED, advance=False, **search), reps)
        restore()
        act = bb.sample_mcts(seed=SEED, advance=False, **search)
        if not torch.equal(act, tree["best"]):
            raise SystemExit("%s: sample_mcts is not mcts's best (S=%d, R=%d, W=%d)" % (TOOL, S, R, W))
        _check_sample(st, act.cpu().numpy(), S, R, W, min(sample, B))
        out_s = bb.step_single(seat, ranks, SEED, rank=True, opponent="mcts", **search)
        ms_step, step_range = _timed(restore, lambda: bb.step_single(seat, ranks, SEED, rank=True, out=out_s, opponent="mcts", **search),
                                     reps)
        opp_plies = float((bb.tcount.to(torch.int64) - keep["tcount"].to(torch.int64) - 1).clamp(min=0).double().mean())
        searched = _check_step(st, seat_np, ranks_np, bb, S, R, W, min(sample, B))
        ms_roll, roll_range = _timed(restore, lambda: bb.rollout_mcts(rollout_plies, seed=SEED, **search), reps)
        floor = 3 * ms_mcts + ms_random
        row = {"game": "blokus", "B": B, "S": S, "W": W, "R": R, "noise": 0.0, "positions": "after %d random plies" % plies,
               "mapping": "workgroup per game" if R >= 4 else "wave per game", "reps": reps,
               "mcts_ms": round(ms_mcts, 4), "mcts_ms_range": [round(x, 4) for x in mcts_range],
               "sample_ms": round(ms_sample, 4), "sample_ms_range": [round(x, 4) for x in sample_range],
               "sample_over_mcts": round(ms_sample / ms_mcts, 3),
               "step_ms": round(ms_step, 4), "step_ms_range": [round(x, 4) for x in step_range],
               "opponent_plies_per_game": round(opp_plies, 3), "searches_in_sampled_games": round(searched, 2),
               "step_random_ms": round(ms_random, 4), "floor_ms": round(floor, 4), "step_over_floor": round(ms_step / floor, 3),
               "rollout_plies": rollout_plies, "rollout_ms": round(ms_roll, 4), "rollout_ms_range": [round(x, 4) for x in roll_range],
               "rollout_plies_per_s": round(B * rollout_plies / ms_roll * 1e3)}
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
    ap.add_argument("--rollout-plies", type=int, default=8, help="plies of the timed rollout_mcts")
    ap.add_argument("--sample", type=int, default=1, help="games the restatement replays")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blokus_mcts_agent_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 32 positions after 48 plies, 8 simulations, W = 4, R = 1 and 4, "
                                                        "2 rollout plies")
    args = ap.parse_args()
    M.require_gpu(TOOL)
    import torch
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of(32, 8, 4, [1, 4], 48, 1, 1, 2)
    else:
        rows = rows_of(args.batch, args.simulations, args.width, [1, 16], args.plies, args.reps, args.sample, args.rollout_plies)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
