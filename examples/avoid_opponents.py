#!/usr/bin/env python3
"""One learner against scripted opponents, B games at once: TronSinglePlayerVectorEnv, the batched counterpart of the
reference's TronRaySinglePlayerEnvironment with its default SimpleAvoidAgent opponents (all on the GPU, no host sync per
step).  The "learner" here is a stand-in policy that turns at random 10 % of the time; plug a network in its place.
Then the same agents in fused rollouts: mean episode length of avoid agents against random agents.

    python examples/avoid_opponents.py [games=4096] [steps=200]
"""
import sys
if "-h" in sys.argv[1:] or "--help" in sys.argv[1:]:
    print(__doc__)
    sys.exit(0)
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from colosseumrl_amd.batched import TronBatch  # noqa: E402
from colosseumrl_amd.vector import TronSinglePlayerVectorEnv  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 200
env = TronSinglePlayerVectorEnv(board_size=15, num_players=4, batch=B, noise=0.1, seed=1)
obs = env.reset()                                        # player 0's observation: board [B, 15, 15], heads / directions / deaths [4, B]
ret = torch.zeros(B, dtype=torch.int64, device=env.batch.device)
episodes = torch.zeros(B, dtype=torch.int64, device=env.batch.device)
for _ in range(K):
    turn = torch.randint(1, 3, (B,), device=env.batch.device)
    action = torch.where(torch.rand(B, device=env.batch.device) < 0.1, turn, torch.zeros_like(turn))   # 0 fwd, 1 right, 2 left
    obs, reward, done, info = env.step(action)
    ret += reward.to(torch.int64)
    episodes += done.to(torch.int64)
print("learner vs avoid agents, %d games x %d steps: %d episodes, mean return per episode %.2f"
      % (B, K, int(episodes.sum()), ret.sum().item() / max(1, int(episodes.sum()))))

for name, run in (("avoid", lambda tb: tb.rollout_avoid(1024, seed=0, noise=0.1)), ("random", lambda tb: tb.rollout(1024, seed=0))):
    tb = TronBatch(board_size=19, num_players=4, batch=B)
    run(tb)
    rows = tb.results()                                  # same rows for both agents: n_episodes, len_sum, last_winners, wins, returns
    print("19x19 P4 %-6s agents: mean episode length %.1f" % (name, rows[:, 1].sum().item() / max(1, rows[:, 0].sum().item())))
