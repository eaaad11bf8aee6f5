"""Tree search next to flat Monte Carlo: a masked-uniform learner, a flat Monte Carlo learner and a search learner
(``mcts_action``, one launch per move for the whole batch), each in ``TicTacToeSinglePlayerVectorEnv`` against the random
and against the noise-free tactical (win-or-block) opponent -- at both seats of 3x3 and at seat 1 of the three-player 3x5
board.  The search and flat Monte Carlo get the same number of playouts per move.  Prints win / draw / loss rates over each
game's first finished episode.  Flat Monte Carlo values every reply as if the opponent played at random; the tree finds
the replies that refute a move.

    python examples/ttt_mcts.py [--batch 4096] [--simulations 128] [--playouts 16] [--exploration 1.0]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv  # noqa: E402

LEARNERS = ("uniform", "flat_mc", "mcts")
BOARDS = [((3, 3), 3, 2, 0), ((3, 3), 3, 2, 1), ((3, 5), 3, 3, 1)]          # dims, K, P, the learner's seat


def first_episodes(board, opponent, batch, simulations, playouts, exploration, learner):
    """(win, draw, loss) rates of the learner over every game's first finished episode, and how many finished"""
    dims, k, p, seat = board
    env = TicTacToeSinglePlayerVectorEnv(dims, k, p, batch, seat=seat, seed=seat + 1, device="cuda", opponent=opponent, noise=0.0)
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
    for step in range((cells + p - 1) // p + 1):        # step_single leaves each game at the learner's turn
        _, reward, done, _ = env.step(policy(step))
        d = done != 0
        result = torch.where(d & ~first, reward, result)
        first |= d
    r = result[first]
    return [float((r == v).float().mean()) for v in (1, 0, -1)], int(first.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--playouts", type=int, default=16)
    ap.add_argument("--exploration", type=float, default=1.0)
    args = ap.parse_args()
    for board in BOARDS:
        for opponent in ("random", "tactical"):
            for learner in LEARNERS:
                (w, d, l), n = first_episodes(board, opponent, args.batch, args.simulations, args.playouts, args.exploration, learner)
                print("tictactoe %s P%d against %-8s %-8s learner at seat %d: win %.3f  draw %.3f  loss %.3f  (%d games)"
                      % ("x".join(map(str, board[0])), board[2], opponent + ",", learner, board[3], w, d, l, n))


if __name__ == "__main__":
    main()
