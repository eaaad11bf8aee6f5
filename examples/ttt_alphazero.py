"""An AlphaZero-style loop on 3x3 TicTacToe with the network-valued tree search (``TTTBatch.puct``): a small torch MLP
(board -> policy logits, one value per player) plays the batch against itself, every move a search of --simulations
descents whose leaves the network values (two launches per simulation for the whole batch, the trees in HBM); the root's
visit counts are the policy target and the final outcomes the value target.  Prints the learner's first-episode loss rate
at seat 1 against the noise-free tactical (win-or-block) opponent before and after the iterations.  One run is one run: the
figures it prints are what that run measured, nothing more.

    python examples/ttt_alphazero.py [--batch 1024] [--iterations 4] [--simulations 32] [--epochs 4] [--eval-games 1024]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from colosseumrl_amd.batched import TTTBatch  # noqa: E402
from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv  # noqa: E402

DIMS, K, P, CELLS = (3, 3), 3, 2, 9


class Net(torch.nn.Module):
    def __init__(self, hidden=64):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Linear(CELLS * P, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden), torch.nn.ReLU())
        self.policy, self.value = torch.nn.Linear(hidden, CELLS), torch.nn.Linear(hidden, P)

    def forward(self, board):
        """board int8 [B, cells] relative to the mover (-1 empty) -> (policy logits [B, cells], value logits [B, P])"""
        planes = torch.stack([(board == p) for p in range(P)], dim=2).flatten(1).float()
        h = self.body(planes)
        return self.policy(h), self.value(h)


def evaluator(net):
    """the search's evaluator: leaves -> (policy weights, values in [0, 1] of the leaf's mover and the players after it)"""
    def evaluate(leaves):
        with torch.no_grad():
            logits, value = net(leaves["board"])
        return torch.softmax(logits, dim=1), torch.sigmoid(value)
    return evaluate


def self_play(net, batch, simulations, seed):
    """one batch of self-play games -> (boards int8 [N, cells], policy targets float [N, cells], value targets float [N, P])"""
    tb = TTTBatch(DIMS, K, P, batch, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    boards, targets, movers, lives = [], [], [], []
    root = None
    for _ in range(CELLS):
        live = (tb.winner < 0) & (tb.valid_mask() != 0)
        root = tb.puct(evaluator(net), simulations, out=root)
        visits = root["visits"].float()
        boards.append(tb.board(tb.to_move)), movers.append(tb.to_move.clone()), lives.append(live)
        targets.append(visits / visits.sum(dim=1, keepdim=True).clamp_min(1.0))
        pick = torch.multinomial(visits + (visits.sum(dim=1, keepdim=True) == 0).float(), 1, generator=gen).squeeze(1)
        tb.step(torch.where(live, pick, torch.full_like(pick, -1)).to(torch.int8))
    winner = tb.winner.to(torch.int64)                                   # -1: a draw
    values = []
    for m in movers:
        seats = (m.to(torch.int64).view(-1, 1) + torch.arange(P, device="cuda").view(1, -1)) % P
        values.append(torch.where(winner.view(-1, 1) < 0, 0.5, (seats == winner.view(-1, 1)).float()))
    keep = torch.cat(lives)
    return torch.cat(boards)[keep], torch.cat(targets)[keep], torch.cat(values)[keep]


def train(net, opt, boards, policy, value, epochs):
    for _ in range(epochs):
        logits, v = net(boards)
        loss = -(policy * torch.log_softmax(logits, dim=1)).sum(dim=1).mean() + torch.nn.functional.binary_cross_entropy_with_logits(v, value)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return float(loss)


def loss_rate(net, games, simulations):
    """the share of first episodes the search learner at seat 1 loses to the noise-free tactical opponent"""
    env = TicTacToeSinglePlayerVectorEnv(DIMS, K, P, games, seat=1, seed=3, device="cuda", opponent="tactical", noise=0.0)
    env.reset()
    first = torch.zeros(games, dtype=torch.bool, device="cuda")
    result = torch.zeros(games, dtype=torch.int8, device="cuda")
    for _ in range(CELLS // P + 1):
        _, reward, done, _ = env.step(env.puct_action(evaluator(net), simulations))
        d = done != 0
        result = torch.where(d & ~first, reward, result)
        first |= d
    return float((result[first] < 0).float().mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--simulations", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--eval-games", type=int, default=1024)
    args = ap.parse_args()
    torch.manual_seed(0)
    net = Net().to("cuda")
    opt = torch.optim.Adam(net.parameters(), lr=3e-3)
    print("loss rate against tactical, seat 1, before: %.3f (%d games, %d simulations a move)"
          % (loss_rate(net, args.eval_games, args.simulations), args.eval_games, args.simulations))
    for it in range(args.iterations):
        boards, policy, value = self_play(net, args.batch, args.simulations, seed=it)
        loss = train(net, opt, boards, policy, value, args.epochs)
        print("iteration %d: boards %s policy targets %s values %s, loss %.4f"
              % (it + 1, tuple(boards.shape), tuple(policy.shape), tuple(value.shape), loss))
    print("loss rate against tactical, seat 1, after %d iterations: %.3f" % (args.iterations, loss_rate(net, args.eval_games, args.simulations)))


if __name__ == "__main__":
    main()
