"""A learner that searches with ``BlokusSinglePlayerVectorEnv.puct_action`` against three random agents in Blokus, over whole
games: the tree search valued by the caller (``crl_blokus_puct_*``: at most ``--width`` sampled candidates per node, two
launches per simulation, the trees in device memory).  No network is trained here: the priors are uniform over the candidates
and the value of a leaf is the share of ``--playouts`` random playouts each player won from the leaf, run by ``playout`` on a
second stepper loaded from the leaf's ``leaf_*`` state.  ``--evaluator net`` puts a policy-value MLP there instead, in one launch
per simulation (``BlokusBatch.net_pack`` / ``BlokusNet.evaluator()``, ``crl_blokus_net_eval``): ``--layers`` hidden layers of
width ``--hidden``, randomly initialised -- the wiring a trained network would use, not a strong player.  Beside it, with the
same opponents, a uniformly random learner.  Prints the share of games each learner won (alone or tied on top); each game's
first finished episode counts.

    python examples/blokus_puct.py [--batch 128] [--seat 0] [--simulations 16] [--width 8] [--playouts 4] [--tiny]
                                   [--evaluator playout|net] [--hidden 128] [--layers 2]
"""
import argparse
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.batched import BlokusBatch  # noqa: E402
from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv  # noqa: E402


def playout_evaluator(batch, width, playouts):
    """the select dict -> (uniform priors, the players' shares of `playouts` random playouts from the leaf, mover first)"""
    scratch = BlokusBatch(batch, device="cuda")
    ones = torch.ones((batch, width), device="cuda")
    turn = torch.arange(4, device="cuda").view(1, 4)
    calls = itertools.count()

    def evaluate(leaves):
        for name in ("occ", "inv", "score", "round", "to_move"):
            getattr(scratch, name).copy_(leaves["leaf_" + name])
        wins = scratch.playout(playouts, seed=next(calls))["wins"][:, 0, :].to(torch.float32) / playouts
        return ones, torch.gather(wins, 1, (leaves["mover"].to(torch.int64).view(-1, 1).clamp(min=0) + turn) & 3)
    return evaluate


def net_evaluator(hidden, layers):
    """the select dict -> the integer (prior, value) of a randomly initialised MLP packed for ``net_eval``"""
    def linear(n_out, n_in):
        m = torch.nn.Linear(n_in, n_out).to("cuda")
        return m.weight.detach(), m.bias.detach()
    trunk = [linear(hidden, BlokusBatch.NET_FEATURES if i == 0 else hidden) for i in range(layers)]
    return BlokusBatch(1, device="cuda").net_pack(trunk, linear(400, hidden), linear(21, hidden), linear(4, hidden)).evaluator()


def random_policy(env, t):
    """a uniformly drawn legal action of the learner (the pass where it has none)"""
    count = env.batch.valid()
    return env.batch.select((torch.rand(env.num_envs, device="cuda") * count.clamp(min=1)).to(torch.int32))[0].to(torch.int64)


def play(batch, seat, policy, max_steps=40):
    """(win share, games) of the learner at `seat` over every game's first finished episode"""
    env = BlokusSinglePlayerVectorEnv(batch, seat=seat, seed=seat + 5, device="cuda")
    env.reset()
    first = torch.zeros(batch, dtype=torch.bool, device="cuda")
    won = torch.zeros(batch, dtype=torch.bool, device="cuda")
    for t in range(max_steps):
        _, _, done, info = env.step(policy(env, t))
        new = (done != 0) & ~first
        won |= new & (((info["winners"].to(torch.int32) >> seat) & 1) != 0)
        first |= done != 0
    return float(won[first].float().mean()), int(first.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seat", type=int, default=0)
    ap.add_argument("--simulations", type=int, default=16)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--playouts", type=int, default=4)
    ap.add_argument("--evaluator", choices=("playout", "net"), default="playout")
    ap.add_argument("--hidden", type=int, default=128, help="--evaluator net: the MLP's width, a multiple of 16 in 16 .. 256")
    ap.add_argument("--layers", type=int, default=2, help="--evaluator net: its hidden layers, 1 .. 3")
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 16 games, 4 simulations, width 4, 1 playout")
    args = ap.parse_args()
    B, S, W, R = (16, 4, 4, 1) if args.tiny else (args.batch, args.simulations, args.width, args.playouts)
    torch.manual_seed(1)
    evaluate = net_evaluator(args.hidden, args.layers) if args.evaluator == "net" else playout_evaluator(B, W, R)
    valued = "a random %d x %d MLP" % (args.hidden, args.layers) if args.evaluator == "net" else "%d playouts" % R
    learners = (("puct", lambda env, t: env.puct_action(evaluate, S, width=W, seed=1000 + t)), ("random", random_policy))
    print("blokus, %d games at seat %d; puct: S = %d, W = %d, leaves valued by %s" % (B, args.seat, S, W, valued))
    for name, policy in learners:
        share, n = play(B, args.seat, policy)
        print("blokus, %-6s learner at seat %d: win share %.3f  (%d games)" % (name, args.seat, share, n))


if __name__ == "__main__":
    main()
