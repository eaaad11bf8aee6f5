"""Times a simulation of the network-valued TicTacToe search with the evaluator people train with -- select, the policy-value
MLP, backup -- once with examples/ttt_alphazero.py's torch evaluator (one-hot planes, four Linear layers, softmax, sigmoid and
puct_quantize: some twenty small launches) and once with the same weights packed for TTTBatch.net_eval (crl_ttt_net_eval: one
launch), in the same run and process, the two alternating.

Per configuration -- 3x3 P2, 3x5 K3 P3, 3x3x3 P4, 5x5 K4 P3; --batch trees (4,096) from the empty board; S = --simulations
(128); an MLP of --layers (2) hidden layers of width --hidden (64), planes = P -- device-event time after a warm-up:
  * torch_sim_us, hip_sim_us: S x (puct_select, evaluate, puct_backup) between two events, divided by S; the median of --reps
    repetitions and their [min, max] (torch_sim_range_us, hip_sim_range_us), the repetitions of the two alternating
  * hip_faster_beyond_spread: the slowest HIP repetition is faster than the fastest torch repetition
  * net_eval_us: net_eval alone on the last simulation's leaves, S calls back to back
  * pair_us: select + backup with a constant evaluator (no launch between them): the floor
  * pack_us: net_pack (repack) alone, back to back: what a trainer pays per optimiser step
Prints one JSON line per configuration and writes them to --out.

    python tools/ttt_net_rate.py [--reps 5] [--batch 4096] [--simulations 128] [--hidden 64] [--layers 2]
                                 [--out profiles/ttt_net_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"


def _torch_net(cells, P, hidden, layers):
    """examples/ttt_alphazero.py's network for any board: (module, its evaluator for puct)"""
    import torch

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            body, n_in = [], cells * P
            for _ in range(layers):
                body += [torch.nn.Linear(n_in, hidden), torch.nn.ReLU()]
                n_in = hidden
            self.body = torch.nn.Sequential(*body)
            self.policy, self.value = torch.nn.Linear(hidden, cells), torch.nn.Linear(hidden, P)

        def forward(self, board):
            planes = torch.stack([(board == p) for p in range(P)], dim=2).flatten(1).float()
            h = self.body(planes)
            return self.policy(h), self.value(h)
    net = Net().to(DEV)

    def evaluate(leaves):
        with torch.no_grad():
            logits, value = net(leaves["board"])
        return torch.softmax(logits, dim=1), torch.sigmoid(value)
    return net, evaluate


def _layers(net):
    linear = [m for m in net.body if hasattr(m, "weight")]
    return [(m.weight, m.bias) for m in linear], (net.policy.weight, net.policy.bias), (net.value.weight, net.value.bias)


def _simulations(tb, S, evaluate, leaves):
    """microseconds per simulation of S x (select, evaluate, backup) between two events, from a fresh search"""
    import torch
    tb.puct_begin(S)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(S):
        tb.puct_select(1.25, 0.5, out=leaves)
        prior, value = evaluate(leaves)
        if prior.is_floating_point():
            prior, value = tb.puct_quantize(prior, value)
        tb.puct_backup(prior, value)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / S


def rows_of(shapes, B, S, reps, hidden, layers):
    import torch
    from colosseumrl_amd.batched import TTTBatch
    rows = []
    for dims, k, p in shapes:
        torch.manual_seed(0)
        tb = TTTBatch(dims, k, p, B, device=DEV)
        module, torch_eval = _torch_net(tb.n_cells, p, hidden, layers)
        net = tb.net_pack(*_layers(module))
        hip_eval = net.evaluator()
        const = (torch.ones((B, tb.n_cells), dtype=torch.int16, device=DEV), torch.full((B, p), 32768, dtype=torch.int32, device=DEV))
        evaluators = {"torch": torch_eval, "hip": hip_eval, "const": lambda leaves: const}
        tb.puct_begin(S)
        leaves = tb.puct_select(1.25, 0.5)
        times = {name: [] for name in evaluators}
        for rep in range(reps + 1):                                            # the first round is the warm-up of every launch
            for name, fn in evaluators.items():                               # alternating: torch, hip, const, torch, ...
                t = _simulations(tb, S, fn, leaves)
                if rep:
                    times[name].append(t)
        out = tb.net_eval(net, leaves)
        eval_ms = M.median(M.back_to_back(lambda: tb.net_eval(net, leaves, out=out), S, reps, warmup=S))
        pack_ms = M.median(M.back_to_back(lambda: net.repack(*_layers(module)), S, reps, warmup=4))
        (t_med, t_rng), (h_med, h_rng), (c_med, _) = (M.spread(times[name]) for name in ("torch", "hip", "const"))
        row = {"game": "tictactoe", "shape": M.shape_name(dims, k, p), "B": B, "S": S, "positions": "empty board",
               "network": {"planes": p, "hidden": hidden, "layers": layers, "packed_bytes": int(net.packed.numel() * 8)}, "reps": reps,
               "torch_sim_us": round(t_med, 2), "torch_sim_range_us": [round(x, 2) for x in t_rng],
               "hip_sim_us": round(h_med, 2), "hip_sim_range_us": [round(x, 2) for x in h_rng],
               "torch_over_hip": round(t_med / h_med, 3), "hip_faster_beyond_spread": bool(h_rng[1] < t_rng[0]),
               "net_eval_us": round(eval_ms * 1e3, 2), "pair_us": round(c_med, 2), "pack_us": round(pack_ms * 1e3, 2)}
        M.emit(row)
        rows.append(row)
        del tb, net
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ttt_net_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: one shape, 64 trees, 16 simulations, one repetition")
    args = ap.parse_args()
    M.require_gpu("ttt_net_rate.py")
    import torch
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of(M.TTT_SHAPES[:1], 64, 16, 1, args.hidden, args.layers)
    else:
        rows = rows_of(M.TTT_SHAPES, args.batch, args.simulations, args.reps, args.hidden, args.layers)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
