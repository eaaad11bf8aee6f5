"""A tree-search learner for Tron whose leaves are valued by Voronoi territory, not by playouts: at every step the learner
plays the most visited action of a UCT search over its own three actions
(``TronSinglePlayerVectorEnv.mcts_territory_action``: one crl_tron_mcts_territory launch for the whole batch, one tree per
game, the opponents modelled by the avoid agent, one flood per leaf).  In TronSinglePlayerVectorEnv (15x15, 4 players, noise
0.1) it prints, per learner, each game's first-episode return, steps survived and win rate against avoid opponents -- the
territory-leaf search at exploration 0.25, 0.5 and 1.0 beside the playout search of examples/tron_mcts.py and the
territory-greedy, avoid and random learners.

    python examples/tron_mcts_territory.py [--batch 2048] [--simulations 48] [--playouts 8] [--seed 5]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.vector import TronSinglePlayerVectorEnv  # noqa: E402


def first_episode(policy, batch, seed, max_t=400):
    """(mean return, mean steps survived, win rate) of every game's first episode"""
    env = TronSinglePlayerVectorEnv(15, 4, batch, noise=0.1, seed=seed, device="cuda")
    env.reset()
    ret = torch.zeros(batch, dtype=torch.int64, device="cuda")
    steps = torch.zeros_like(ret)
    won = torch.zeros(batch, dtype=torch.bool, device="cuda")
    live = torch.ones(batch, dtype=torch.bool, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for t in range(max_t):
        _, reward, done, _ = env.step(policy(env, t, gen))
        ret += torch.where(live, reward.to(torch.int64), 0)
        steps += live.to(torch.int64)
        won |= live & (reward == 10)
        live &= done == 0
        if t % 20 == 19 and not bool(live.any()):
            break
    return ret.double().mean().item(), steps.double().mean().item(), won.double().mean().item()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--simulations", type=int, default=48)
    ap.add_argument("--playouts", type=int, default=8, help="playouts per leaf of the playout search")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()

    def leaves(exploration):
        return lambda env, t, gen: env.mcts_territory_action(a.simulations, seed=1000 + t, exploration=exploration)

    def playouts(env, t, gen):
        return env.mcts_action(a.simulations, a.playouts, seed=1000 + t)

    def territory(env, t, gen):
        return env.territory_action()

    def uniform(env, t, gen):
        return torch.randint(0, 3, (env.num_envs,), device="cuda", generator=gen)

    def avoid(env, t, gen):
        act = env.batch.sample_avoid(99, env.noise, players=[0], advance=False)[0].to(torch.int64)
        return torch.where(act < 0, 2, act)

    print("opponents: avoid; the searches: %d simulations, the playout search with %d playouts per leaf" % (a.simulations, a.playouts))
    print("learner           return   steps   win rate   (first episode, %d games)" % a.batch)
    for name, pol in (("leaves-0.25", leaves(0.25)), ("leaves-0.5", leaves(0.5)), ("leaves-1.0", leaves(1.0)), ("mcts", playouts),
                      ("territory", territory), ("avoid", avoid), ("random", uniform)):
        r, s, w = first_episode(pol, a.batch, a.seed)
        print("%-15s %8.2f %7.1f %9.3f" % (name, r, s, w))


if __name__ == "__main__":
    main()
