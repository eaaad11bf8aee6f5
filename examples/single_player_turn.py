"""One learner against the random agent in the turn-based games: a masked-uniform learner (a uniformly drawn legal move)
in TicTacToeSinglePlayerVectorEnv and BlokusSinglePlayerVectorEnv, its win / draw rates printed per seat.

    python examples/single_player_turn.py [--ttt-batch 65536] [--blokus-batch 2048]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv, TicTacToeSinglePlayerVectorEnv  # noqa: E402


def ttt_rates(batch, seat, steps=12):
    env = TicTacToeSinglePlayerVectorEnv((3, 3), 3, 2, batch, seat=seat, seed=1, device="cuda")
    env.reset()
    valid = env.batch.valid_mask()
    bits = 1 << torch.arange(9, device="cuda", dtype=torch.int32)
    wins = draws = episodes = 0
    for _ in range(steps):
        free = (valid[:, None] & bits[None, :]) != 0
        action = torch.rand((batch, 9), device="cuda").masked_fill(~free, -1.0).argmax(dim=1)
        _, reward, done, info = env.step(action)
        d = done != 0
        episodes += int(d.sum())
        wins += int((d & (reward == 1)).sum())
        draws += int((d & (reward == 0)).sum())
        valid = info["valid"].clone()
    return wins / episodes, draws / episodes, episodes


def blokus_rates(batch, seat, steps=60):
    # rank actions: a uniform index into the learner's legal list, no list needed
    env = BlokusSinglePlayerVectorEnv(batch, seat=seat, seed=2, action="rank", device="cuda")
    env.reset()
    n_valid = env.batch.valid(player=env.seat)
    wins = draws = episodes = 0
    me = 1 << seat
    for _ in range(steps):
        rank = (torch.rand(batch, device="cuda") * n_valid.clamp(min=1).double()).long()
        _, reward, done, info = env.step(rank)
        d = done != 0
        w = info["winners"].to(torch.int32)           # bitmask of the players with the best score
        episodes += int(d.sum())
        wins += int((d & (w == me)).sum())
        draws += int((d & ((w & me) != 0) & (w != me)).sum())
        n_valid = info["n_valid"].clone()
    return wins / max(episodes, 1), draws / max(episodes, 1), episodes


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ttt-batch", type=int, default=65536)
    ap.add_argument("--blokus-batch", type=int, default=2048)
    args = ap.parse_args()
    for seat in (0, 1):
        win, draw, n = ttt_rates(args.ttt_batch, seat)
        print("tictactoe 3x3, learner at seat %d: win %.3f  draw %.3f  loss %.3f  (%d episodes)" % (seat, win, draw, 1 - win - draw, n))
    for seat in range(4):
        win, draw, n = blokus_rates(args.blokus_batch, seat)
        print("blokus, learner at seat %d: win %.3f  draw (best score shared) %.3f  (%d episodes)" % (seat, win, draw, n))


if __name__ == "__main__":
    main()
