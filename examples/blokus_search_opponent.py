"""The Blokus tree search as the opponents of a learner: ``BlokusSinglePlayerVectorEnv(opponent="mcts")`` seats
``crl_blokus_step_single_mcts``'s search agent in the three other seats, one launch per step.  Three learners -- uniformly
random, flat Monte Carlo (``BlokusBatch.flat_mc_action`` over ``--width`` drawn candidates) and the tree search
(``mcts_action``) with the same number of playouts per move -- play whole games at each seat against three random agents and
against three seated searches of the same strength.  Prints, per opponent, learner and seat, the share of games the learner
won (alone or tied on top) and its mean final rank (3 = best).  Each game's first finished episode counts.

    python examples/blokus_search_opponent.py [--batch 128] [--simulations 32] [--playouts 1] [--width 8] [--noise 0.0] [--tiny]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv  # noqa: E402

LEARNERS = ("random", "flat_mc", "mcts")
OPPONENTS = ("random", "mcts")


def play(batch, seat, learner, opponent, S, R, W, noise, max_steps=30):
    """(win share, mean final rank, games) of `learner` at `seat` against three `opponent`s, over every game's first episode"""
    env = BlokusSinglePlayerVectorEnv(batch, seat=seat, seed=seat + 5, device="cuda", opponent=opponent, noise=noise,
                                      simulations=S, playouts=R, width=W)
    bb = env.batch

    def drawn(n):
        """n uniformly drawn legal ids per game (repeats possible; -1 where the learner must pass)"""
        _, count = bb.select(torch.zeros(batch, dtype=torch.int32, device="cuda"))
        rank = (torch.rand((batch, n), device="cuda") * count.clamp(min=1)[:, None]).to(torch.int32)
        return torch.stack([bb.select(rank[:, a].contiguous())[0] for a in range(n)], dim=1).contiguous()

    def policy(t):
        if learner == "random":
            return drawn(1)[:, 0].to(torch.int64)
        if learner == "flat_mc":
            return bb.flat_mc_action(drawn(W), max(1, S * R // W), seed=23 + t)
        return env.mcts_action(S, R, W, seed=23 + t)
    env.reset()
    first = torch.zeros(batch, dtype=torch.bool, device="cuda")
    rank = torch.zeros(batch, dtype=torch.int8, device="cuda")
    won = torch.zeros(batch, dtype=torch.bool, device="cuda")
    seats = env.seat.to(torch.int32)
    for t in range(max_steps):
        _, reward, done, info = env.step(policy(t))
        new = (done != 0) & ~first
        rank = torch.where(new, reward, rank)
        won = torch.where(new, ((info["winners"].to(torch.int32) >> seats) & 1) != 0, won)
        first |= done != 0
    n = int(first.sum())
    return float(won[first].float().mean()), float(rank[first].float().mean()), n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--simulations", type=int, default=32)
    ap.add_argument("--playouts", type=int, default=1)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--noise", type=float, default=0.0, help="the seated searches play the random agent's move with this probability")
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 16 games, 8 simulations, width 4")
    args = ap.parse_args()
    B, S, R, W = (16, 8, 1, 4) if args.tiny else (args.batch, args.simulations, args.playouts, args.width)
    torch.manual_seed(1)
    print("blokus, %d games per seat, %d playouts per move (S = %d, R = %d, W = %d), learners and seated searches alike"
          % (B, S * R, S, R, W))
    for opponent in OPPONENTS:
        for learner in LEARNERS:
            total_w, total_r = 0.0, 0.0
            for seat in range(4):
                w, r, n = play(B, seat, learner, opponent, S, R, W, args.noise)
                total_w, total_r = total_w + w / 4, total_r + r / 4
                print("blokus, against 3 x %-6s: %-7s learner at seat %d: win share %.3f  mean final rank %.2f of 3  (%d games)"
                      % (opponent, learner, seat, w, r, n))
            print("blokus, against 3 x %-6s: %-7s learner, all seats : win share %.3f  mean final rank %.2f of 3"
                  % (opponent, learner, total_w, total_r))


if __name__ == "__main__":
    main()
