"""A flat Monte Carlo learner against the random agent in the turn-based games: at its turn the learner plays the
candidate with the most playout wins (``TTTBatch`` / ``BlokusBatch.flat_mc_action``, one playout launch), in
TicTacToeSinglePlayerVectorEnv and BlokusSinglePlayerVectorEnv.  Prints win / draw / loss rates per seat (Blokus: the
mean final rank, 3 = best) next to those of a uniformly random learner.  Each game's first finished episode counts.

    python examples/flat_mc.py [--ttt-batch 16384] [--ttt-playouts 256] [--blokus-batch 256] [--blokus-candidates 16]
                               [--blokus-playouts 8]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv, TicTacToeSinglePlayerVectorEnv  # noqa: E402


def _first_episodes(env, policy, max_steps):
    """reward of every game's first finished episode: step_single leaves each game at the learner's turn"""
    B = env.num_envs
    env.reset()
    first = torch.zeros(B, dtype=torch.bool, device="cuda")
    result = torch.zeros(B, dtype=torch.int8, device="cuda")
    for _ in range(max_steps):
        _, reward, done, _ = env.step(policy())
        d = done != 0
        result = torch.where(d & ~first, reward, result)
        first |= d
    return result[first], int(first.sum())


def ttt(batch, playouts, seat, learner):
    env = TicTacToeSinglePlayerVectorEnv((3, 3), 3, 2, batch, seat=seat, seed=seat + 1, device="cuda")
    bits = 1 << torch.arange(9, device="cuda", dtype=torch.int32)

    def random_policy():
        free = (env.batch.valid_mask()[:, None] & bits[None, :]) != 0
        return torch.rand((batch, 9), device="cuda").masked_fill(~free, -1.0).argmax(dim=1)

    def mc_policy():
        return env.batch.flat_mc_action(playouts, seed=17)
    r, n = _first_episodes(env, mc_policy if learner == "flat_mc" else random_policy, 6)
    return float((r == 1).float().mean()), float((r == 0).float().mean()), float((r == -1).float().mean()), n


def blokus(batch, n_cand, playouts, seat, learner):
    env = BlokusSinglePlayerVectorEnv(batch, seat=seat, seed=seat + 5, device="cuda")
    bb = env.batch

    def random_ranks():
        _, count = bb.select(torch.zeros(batch, dtype=torch.int32, device="cuda"))
        return (torch.rand((batch, n_cand), device="cuda") * count.clamp(min=1)[:, None]).to(torch.int32), count

    def random_policy():
        rank, count = random_ranks()
        act = bb.select(rank[:, 0].contiguous())[0]
        return act.to(torch.int64)

    def mc_policy():
        rank, _ = random_ranks()                  # A random legal ids (repeats possible; -1 where there is none)
        cand = torch.stack([bb.select(rank[:, a].contiguous())[0] for a in range(n_cand)], dim=1).contiguous()
        return bb.flat_mc_action(cand, playouts, seed=23)
    r, n = _first_episodes(env, mc_policy if learner == "flat_mc" else random_policy, 30)
    return float(r.float().mean()), n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ttt-batch", type=int, default=16384)
    ap.add_argument("--ttt-playouts", type=int, default=256)
    ap.add_argument("--blokus-batch", type=int, default=256)
    ap.add_argument("--blokus-candidates", type=int, default=16)
    ap.add_argument("--blokus-playouts", type=int, default=8)
    args = ap.parse_args()
    for seat in (0, 1):
        for learner in ("flat_mc", "random"):
            w, d, l, n = ttt(args.ttt_batch, args.ttt_playouts, seat, learner)
            print("tictactoe 3x3, %-7s learner at seat %d: win %.3f  draw %.3f  loss %.3f  (%d games)" % (learner, seat, w, d, l, n))
    for seat in range(4):
        for learner in ("flat_mc", "random"):
            rank, n = blokus(args.blokus_batch, args.blokus_candidates, args.blokus_playouts, seat, learner)
            print("blokus, %-7s learner at seat %d: mean final rank %.2f of 3  (%d games)" % (learner, seat, rank, n))


if __name__ == "__main__":
    main()
