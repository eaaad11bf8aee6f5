"""The tree search as an opponent: a masked-uniform learner, a flat Monte Carlo learner and a search learner
(``mcts_action``), each in ``TicTacToeSinglePlayerVectorEnv`` against the random, the noise-free tactical (win-or-block) and
the noise-free search opponent (``opponent="mcts"``: one launch per learner step, a wave per game) -- at both seats of 3x3.
Prints win / draw / loss rates over each game's first finished episode, and at the end the outcome of search self-play
(``TTTBatch.rollout_mcts``).  The tactical agent blocks one threat; the search also sees the forks that make two.

    python examples/ttt_search_opponent.py [--batch 4096] [--simulations 64] [--playouts 16] [--exploration 1.0]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.batched import TTTBatch  # noqa: E402
from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv  # noqa: E402

LEARNERS = ("uniform", "flat_mc", "mcts")
OPPONENTS = ("random", "tactical", "mcts")
DIMS, K, P = (3, 3), 3, 2


def first_episodes(seat, opponent, batch, simulations, playouts, exploration, learner):
    """(win, draw, loss) rates of the learner over every game's first finished episode, and how many finished"""
    search = dict(simulations=simulations, playouts=playouts, exploration=exploration) if opponent == "mcts" else {}
    env = TicTacToeSinglePlayerVectorEnv(DIMS, K, P, batch, seat=seat, seed=seat + 1, device="cuda", opponent=opponent, noise=0.0,
                                         **search)
    cells = env.batch.n_cells
    bits = 1 << torch.arange(cells, device="cuda", dtype=torch.int32)
    per_cell = -(-simulations * playouts // cells)      # flat Monte Carlo: the search's budget spread over the cells

    def policy(step):
        if learner == "uniform":
            free = (env.batch.valid_mask()[:, None] & bits[None, :]) != 0
            return torch.rand((batch, cells), device="cuda").masked_fill(~free, -1.0).argmax(dim=1)
        if learner == "flat_mc":
            return env.batch.flat_mc_action(per_cell, seed=17 + step)
        return env.mcts_action(simulations, playouts, seed=17 + step, exploration=exploration)
    env.reset()
    first = torch.zeros(batch, dtype=torch.bool, device="cuda")
    result = torch.zeros(batch, dtype=torch.int8, device="cuda")
    for step in range((cells + P - 1) // P + 1):        # step_single leaves each game at the learner's turn
        _, reward, done, _ = env.step(policy(step))
        d = done != 0
        result = torch.where(d & ~first, reward, result)
        first |= d
    r = result[first]
    return [float((r == v).float().mean()) for v in (1, 0, -1)], int(first.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=64)
    ap.add_argument("--playouts", type=int, default=16)
    ap.add_argument("--exploration", type=float, default=1.0)
    args = ap.parse_args()
    for seat in (0, 1):
        for opponent in OPPONENTS:
            for learner in LEARNERS:
                (w, d, l), n = first_episodes(seat, opponent, args.batch, args.simulations, args.playouts, args.exploration, learner)
                print("tictactoe 3x3 against %-9s %-8s learner at seat %d: win %.3f  draw %.3f  loss %.3f  (%d games)"
                      % (opponent + ",", learner, seat, w, d, l, n))
    tb = TTTBatch(DIMS, K, P, args.batch, device="cuda")
    tb.rollout_mcts(18, args.simulations, args.playouts, seed=3, exploration=args.exploration)
    res = tb.results().to(torch.float64).sum(dim=0)     # n_episodes, len_sum, draw_count, win_count[P]
    print("self-play of the search, 18 plies in every game: %d episodes, first player wins %.3f, second %.3f, draws %.3f"
          % (int(res[0]), float(res[3] / res[0]), float(res[4] / res[0]), float(res[2] / res[0])))


if __name__ == "__main__":
    main()
