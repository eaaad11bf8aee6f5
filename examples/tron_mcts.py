"""A tree-search learner for Tron: at every step the learner plays the most visited action of a UCT search over its own
three actions (``TronSinglePlayerVectorEnv.mcts_action``: one crl_tron_mcts launch for the whole batch, one tree per game,
the opponents modelled by the avoid agent, the leaves valued by avoid-agent playouts).  In TronSinglePlayerVectorEnv (15x15,
4 players, noise 0.1) it prints, per learner, each game's first-episode return, steps survived and win rate against avoid
opponents -- the search learner beside the territory, flat Monte Carlo, avoid and random learners of
examples/tron_territory.py; flat Monte Carlo gets the search's playouts per move (simulations x playouts / 3 per action).

    python examples/tron_mcts.py [--batch 2048] [--simulations 48] [--playouts 8] [--seed 5]
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
    ap.add_argument("--playouts", type=int, default=8)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    flat_r = -(-a.simulations * a.playouts // 3)

    def search(env, t, gen):
        return env.mcts_action(a.simulations, a.playouts, seed=1000 + t)

    def territory(env, t, gen):
        return env.territory_action()

    def flat_mc(env, t, gen):
        return env.flat_mc_action(flat_r, seed=1000 + t)

    def uniform(env, t, gen):
        return torch.randint(0, 3, (env.num_envs,), device="cuda", generator=gen)

    def avoid(env, t, gen):
        act = env.batch.sample_avoid(99, env.noise, players=[0], advance=False)[0].to(torch.int64)
        return torch.where(act < 0, 2, act)

    print("opponents: avoid; the search: %d simulations x %d playouts, flat MC: %d playouts per action" % (a.simulations, a.playouts, flat_r))
    print("learner      return   steps   win rate   (first episode, %d games)" % a.batch)
    for name, pol in (("mcts", search), ("territory", territory), ("flat MC", flat_mc), ("avoid", avoid), ("random", uniform)):
        r, s, w = first_episode(pol, a.batch, a.seed)
        print("%-10s %8.2f %7.1f %9.3f" % (name, r, s, w))


if __name__ == "__main__":
    main()
