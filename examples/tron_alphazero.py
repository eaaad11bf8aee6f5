"""An AlphaZero-style loop on Tron with the network-valued tree search (``TronBatch.puct``): a small torch network (the
learner's relative observation -> policy logits over forward / right / left, one value) plays seat 0 of a batch of games
against avoid-agent opponents (``TronSinglePlayerVectorEnv``), every move a search of --simulations descents whose leaves
the network values (two launches per simulation for the whole batch, the trees in HBM, the opponents modelled by the avoid
agent inside the tree); the root's visit counts are the policy target and the episode's outcome (1 = the learner survived
as the winner) the value target.  Prints the learner's first-episode win rate before and after the iterations.  One run is
one run: the figures it prints are what that run measured, nothing more.

    python examples/tron_alphazero.py [--size 11] [--players 4] [--batch 512] [--iterations 4] [--simulations 24]
                                      [--epochs 4] [--eval-games 512] [--max-steps 120]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_net(torch, N, P, hidden=128):
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.body = torch.nn.Sequential(torch.nn.Linear(4 * N * N + 4, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden),
                                            torch.nn.ReLU())
            self.policy, self.value = torch.nn.Linear(hidden, 3), torch.nn.Linear(hidden, 1)

        def forward(self, board, heads, dirs):
            """board int8 [B, N*N] relative to the learner (0 empty, 1 its own trail), heads int16 [P, B], dirs int8 [P, B]
            (row 0: the learner's) -> (policy logits [B, 3], value logit [B])"""
            b = board.view(board.shape[0], -1).to(torch.int64)
            head = torch.zeros_like(b).scatter_(1, heads[0].to(torch.int64).clamp(0, N * N - 1).view(-1, 1), 1)
            planes = torch.cat([(b == 0), (b == 1), (b > 1), head != 0], dim=1).float()
            facing = torch.nn.functional.one_hot(dirs[0].to(torch.int64) & 3, 4).float()
            h = self.body(torch.cat([planes, facing], dim=1))
            return self.policy(h), self.value(h).squeeze(1)
    return Net()


def evaluator(torch, net):
    """the search's evaluator: leaves -> (policy weights, the seat's value in [0, 1])"""
    def evaluate(leaves):
        with torch.no_grad():
            logits, value = net(leaves["obs_board"], leaves["obs_heads"], leaves["obs_dirs"])
        return torch.softmax(logits, dim=1), torch.sigmoid(value)
    return evaluate


def episodes(torch, net, args, games, seed, sample):
    """every game's first episode with the search learner: (boards, heads, dirs, policy targets, value targets) of the
    learner's positions, and the share of episodes it won.  sample: draw the move from the visit counts (self-play) or take
    the most visited (evaluation)."""
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    env = TronSinglePlayerVectorEnv(args.size, args.players, games, noise=0.1, seed=seed, device="cuda")
    env.reset()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    over = torch.zeros(games, dtype=torch.bool, device="cuda")
    won = torch.zeros(games, dtype=torch.bool, device="cuda")
    kept, root = [], None
    for t in range(args.max_steps):
        b = env.batch
        root = b.puct(evaluator(torch, net), args.simulations, seed=1000 + t, agent="avoid", noise=env.noise, out=root)
        visits = root["visits"].float()
        total = visits.sum(dim=1, keepdim=True)
        kept.append((b.board.clone(), b.heads.clone(), b.dirs.clone(), visits / total.clamp_min(1.0), (~over) & (total.view(-1) > 0)))
        if sample:
            act = torch.multinomial(visits + (total == 0).float(), 1, generator=gen).squeeze(1)
        else:
            act = root["best"].to(torch.int64).clamp_min(0)
        _, reward, done, _ = env.step(act)
        fresh = (done != 0) & ~over
        won |= fresh & (reward == 10)
        over |= fresh
        if (t + 1) % 20 == 0 and bool(over.all()):
            break
    live = torch.cat([k[4] for k in kept])
    boards, pol = torch.cat([k[0] for k in kept])[live], torch.cat([k[3] for k in kept])[live]
    heads, dirs = torch.cat([k[1] for k in kept], dim=1)[:, live], torch.cat([k[2] for k in kept], dim=1)[:, live]
    value = torch.cat([won.float() for _ in kept])[live]
    return (boards, heads, dirs, pol, value), float(won.float().mean())


def train(torch, net, opt, data, epochs):
    boards, heads, dirs, policy, value = data
    for _ in range(epochs):
        logits, v = net(boards, heads, dirs)
        loss = -(policy * torch.log_softmax(logits, dim=1)).sum(dim=1).mean() + torch.nn.functional.binary_cross_entropy_with_logits(v, value)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return float(loss)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=11)
    ap.add_argument("--players", type=int, default=4)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--simulations", type=int, default=24)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--eval-games", type=int, default=512)
    ap.add_argument("--max-steps", type=int, default=120)
    args = ap.parse_args()
    import torch
    torch.manual_seed(0)
    net = make_net(torch, args.size, args.players).to("cuda")
    opt = torch.optim.Adam(net.parameters(), lr=3e-3)
    _, rate = episodes(torch, net, args, args.eval_games, 3, sample=False)
    print("win rate against %d avoid opponents, before: %.3f (%d games, %d simulations a move)"
          % (args.players - 1, rate, args.eval_games, args.simulations))
    for it in range(args.iterations):
        data, played = episodes(torch, net, args, args.batch, 100 + it, sample=True)
        loss = train(torch, net, opt, data, args.epochs)
        print("iteration %d: boards %s policy targets %s values %s, self-play win rate %.3f, loss %.4f"
              % (it + 1, tuple(data[0].shape), tuple(data[3].shape), tuple(data[4].shape), played, loss))
    _, rate = episodes(torch, net, args, args.eval_games, 3, sample=False)
    print("win rate against %d avoid opponents, after %d iterations: %.3f" % (args.players - 1, args.iterations, rate))


if __name__ == "__main__":
    main()
