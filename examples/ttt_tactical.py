"""Learners against TicTacToe's tactical (win-or-block) opponents: a masked-uniform learner, a flat Monte Carlo learner
with random playouts and one with tactical playouts, each in ``TicTacToeSinglePlayerVectorEnv(opponent="tactical")``.
Prints win / draw / loss rates per seat over each game's first finished episode.  Uniform playouts value a position as if
nobody would ever take a winning cell; tactical playouts know that the opponent will.

    python examples/ttt_tactical.py [--batch 16384] [--playouts 256] [--noise 0.1]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv  # noqa: E402

LEARNERS = ("uniform", "flat_mc random", "flat_mc tactical")


def first_episodes(batch, playouts, noise, seat, learner):
    """(win, draw, loss) rates of the learner over every game's first finished episode, and how many finished"""
    env = TicTacToeSinglePlayerVectorEnv((3, 3), 3, 2, batch, seat=seat, seed=seat + 1, device="cuda", opponent="tactical",
                                         noise=noise)
    bits = 1 << torch.arange(9, device="cuda", dtype=torch.int32)

    def policy():
        if learner == "uniform":
            free = (env.batch.valid_mask()[:, None] & bits[None, :]) != 0
            return torch.rand((batch, 9), device="cuda").masked_fill(~free, -1.0).argmax(dim=1)
        return env.batch.flat_mc_action(playouts, seed=17, agent=learner.split()[1], noise=noise)
    env.reset()
    first = torch.zeros(batch, dtype=torch.bool, device="cuda")
    result = torch.zeros(batch, dtype=torch.int8, device="cuda")
    for _ in range(6):                                  # step_single leaves each game at the learner's turn
        _, reward, done, _ = env.step(policy())
        d = done != 0
        result = torch.where(d & ~first, reward, result)
        first |= d
    r = result[first]
    return [float((r == v).float().mean()) for v in (1, 0, -1)], int(first.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--playouts", type=int, default=256)
    ap.add_argument("--noise", type=float, default=0.1)
    args = ap.parse_args()
    for seat in (0, 1):
        for learner in LEARNERS:
            (w, d, l), n = first_episodes(args.batch, args.playouts, args.noise, seat, learner)
            print("tictactoe 3x3 against tactical(noise %.2f), %-16s learner at seat %d: win %.3f  draw %.3f  loss %.3f  (%d games)"
                  % (args.noise, learner, seat, w, d, l, n))


if __name__ == "__main__":
    main()
