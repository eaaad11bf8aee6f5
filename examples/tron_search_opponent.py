"""Tron learners against three kinds of scripted opponents, the strongest of them a tree search: in
``TronSinglePlayerVectorEnv`` (15x15, 4 players, noise 0.1) the three opponents are the avoid agent, the territory-greedy agent
or the territory tree search (``opponent="mcts_territory"``: one crl_tron_sample_mcts_territory launch per step for all three
seats of every game, a tree per seat, the other players modelled by the avoid agent).  It prints the first-episode win rate
of four learners -- uniform, the avoid agent, ``territory_action`` and ``mcts_territory_action`` -- against each of them.

    python examples/tron_search_opponent.py [--batch 2048] [--simulations 48] [--seed 5]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.vector import TronSinglePlayerVectorEnv  # noqa: E402

OPPONENTS = ("avoid", "territory", "mcts_territory")


def first_episode_wins(policy, opponent, batch, simulations, seed, max_t=400):
    """the share of games whose first episode the learner wins"""
    env = TronSinglePlayerVectorEnv(15, 4, batch, noise=0.1, seed=seed, device="cuda", opponent=opponent, simulations=simulations)
    env.reset()
    won = torch.zeros(batch, dtype=torch.bool, device="cuda")
    live = torch.ones(batch, dtype=torch.bool, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for t in range(max_t):
        _, reward, done, _ = env.step(policy(env, t, gen))
        won |= live & (reward == 10)
        live &= done == 0
        if t % 20 == 19 and not bool(live.any()):
            break
    return won.double().mean().item()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--simulations", type=int, default=48, help="of the search opponents and of the search learner")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()

    def uniform(env, t, gen):
        return torch.randint(0, 3, (env.num_envs,), device="cuda", generator=gen)

    def avoid(env, t, gen):
        act = env.batch.sample_avoid(99, env.noise, players=[0], advance=False)[0].to(torch.int64)
        return torch.where(act < 0, 2, act)

    def territory(env, t, gen):
        return env.territory_action()

    def search(env, t, gen):
        return env.mcts_territory_action(a.simulations, seed=1000 + t)

    print("first-episode win rate of the learner (player 0) against three opponents, %d games, the searches: %d simulations"
          % (a.batch, a.simulations))
    print("learner \\ opponents    avoid  territory  mcts_territory")
    for name, pol in (("uniform", uniform), ("avoid", avoid), ("territory", territory), ("search", search)):
        wins = [first_episode_wins(pol, opp, a.batch, a.simulations, a.seed) for opp in OPPONENTS]
        print("%-18s %8.3f %10.3f %15.3f" % ((name,) + tuple(wins)))


if __name__ == "__main__":
    main()
