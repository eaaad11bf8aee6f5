"""Times a simulation of the network-valued Tron search with the evaluator people train with -- select, the policy-value MLP,
backup -- once with examples/tron_alphazero.py's torch evaluator (scatter_, three compares, cat, one_hot, float, four Linear
layers, softmax, sigmoid and puct_quantize: some thirty small launches) and once with the same weights packed for
TronBatch.net_eval (crl_tron_net_eval: one launch), in the same run and process, the two alternating.

Per configuration -- 11x11 P4 with 512 trees (the example's size) and 20x20 P4 with 4,096 trees, or --size / --players / --batch;
trees from the reset position; S = --simulations (64); an MLP of --layers (2) hidden layers of width --hidden (128) --
device-event time after a warm-up:
  * torch_sim_us, hip_sim_us: S x (puct_select, evaluate, puct_backup) between two events, divided by S; the median of --reps
    repetitions and their [min, max] (torch_sim_range_us, hip_sim_range_us), the repetitions of the two alternating
  * hip_faster_beyond_spread: the slowest HIP repetition is faster than the fastest torch repetition
  * net_eval_us: net_eval alone on the last simulation's leaves, S calls back to back
  * pair_us: select + backup with a constant evaluator (no launch between them): the floor
  * pack_us: net_pack (repack) alone, back to back: what a trainer pays per optimiser step
Prints one JSON line per configuration and writes them to --out.

    python tools/tron_net_rate.py [--reps 5] [--simulations 64] [--hidden 128] [--layers 2] [--size N --players P --batch B]
                                  [--out profiles/tron_net_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"
SHAPES = [(11, 4, 512), (20, 4, 4096)]                          # (N, players, trees)


def _torch_net(N, hidden, layers):
    """examples/tron_alphazero.py's network with `layers` hidden layers: (module, its evaluator for puct)"""
    import torch

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            body, n_in = [], 4 * N * N + 4
            for _ in range(layers):
                body += [torch.nn.Linear(n_in, hidden), torch.nn.ReLU()]
                n_in = hidden
            self.body = torch.nn.Sequential(*body)
            self.policy, self.value = torch.nn.Linear(hidden, 3), torch.nn.Linear(hidden, 1)

        def forward(self, board, heads, dirs):
            b = board.view(board.shape[0], -1).to(torch.int64)
            head = torch.zeros_like(b).scatter_(1, heads[0].to(torch.int64).clamp(0, N * N - 1).view(-1, 1), 1)
            planes = torch.cat([(b == 0), (b == 1), (b > 1), head != 0], dim=1).float()
            facing = torch.nn.functional.one_hot(dirs[0].to(torch.int64) & 3, 4).float()
            h = self.body(torch.cat([planes, facing], dim=1))
            return self.policy(h), self.value(h).squeeze(1)
    net = Net().to(DEV)

    def evaluate(leaves):
        with torch.no_grad():
            logits, value = net(leaves["obs_board"], leaves["obs_heads"], leaves["obs_dirs"])
        return torch.softmax(logits, dim=1), torch.sigmoid(value)
    return net, evaluate


def _layers(net):
    linear = [m for m in net.body if hasattr(m, "weight")]
    return [(m.weight, m.bias) for m in linear], (net.policy.weight, net.policy.bias), (net.value.weight, net.value.bias)


def _simulations(tb, S, evaluate, leaves):
    """microseconds per simulation of S x (select, evaluate, backup) between two events, from a fresh search"""
    import torch
    tb.puct_begin(S, agent="avoid")
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


def rows_of(shapes, S, reps, hidden, layers):
    import torch
    from colosseumrl_amd.batched import TronBatch
    rows = []
    for N, p, B in shapes:
        torch.manual_seed(0)
        tb = TronBatch(N, p, B, device=DEV)
        module, torch_eval = _torch_net(N, hidden, layers)
        net = tb.net_pack(*_layers(module))
        hip_eval = net.evaluator()
        const = (torch.ones((B, 3), dtype=torch.int16, device=DEV), torch.full((B,), 32768, dtype=torch.int32, device=DEV))
        evaluators = {"torch": torch_eval, "hip": hip_eval, "const": lambda leaves: const}
        tb.puct_begin(S, agent="avoid")
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
        row = {"game": "tron", "shape": "%dx%d_p%d" % (N, N, p), "B": B, "S": S, "positions": "reset, avoid model",
               "network": {"inputs": 4 * N * N + 4, "hidden": hidden, "layers": layers, "packed_bytes": int(net.packed.numel() * 8)},
               "reps": reps, "torch_sim_us": round(t_med, 2), "torch_sim_range_us": [round(x, 2) for x in t_rng],
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
    ap.add_argument("--simulations", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--size", type=int, default=0, help="one configuration instead of the two: the board size (with --players, --batch)")
    ap.add_argument("--players", type=int, default=4)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tron_net_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 7x7 P2, 64 trees, 8 simulations, one repetition, hidden 32")
    args = ap.parse_args()
    M.require_gpu("tron_net_rate.py")
    import torch
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of([(7, 2, 64)], 8, 1, 32, args.layers)
    else:
        shapes = [(args.size, args.players, args.batch)] if args.size else SHAPES
        rows = rows_of(shapes, args.simulations, args.reps, args.hidden, args.layers)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
