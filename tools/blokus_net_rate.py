"""Times a simulation of the network-valued Blokus search -- select, the policy-value MLP, backup -- once with the network as a
plain torch module (four compares, cat, float, the Linear layers, the decode of the candidate ids and the gather of the cell
map in torch, softmax, sigmoid and puct_quantize: some sixty small launches) and once with the same weights packed for
BlokusBatch.net_eval (crl_blokus_net_eval: one launch), in the same run and process, the two alternating.

Per width W in --widths (16, 64) -- --batch (1,024) trees from mid-game positions (--plies random plies from the reset);
S = --simulations (32); an MLP of --layers (2) hidden layers of width --hidden (128) -- device-event time after a warm-up:
  * torch_sim_us, hip_sim_us: S x (puct_select, evaluate, puct_backup) between two events, divided by S; the median of --reps
    repetitions and their [min, max] (torch_sim_range_us, hip_sim_range_us), the repetitions of the two alternating
  * hip_faster_beyond_spread: the slowest HIP repetition is faster than the fastest torch repetition
  * net_eval_us: net_eval alone on the last simulation's leaves, S calls back to back
  * pair_us: select + backup with a constant evaluator (no launch between them): the floor
  * pack_us: net_pack (repack) alone, back to back: what a trainer pays per optimiser step
Prints one JSON line per width and writes them to --out.

    python tools/blokus_net_rate.py [--reps 5] [--simulations 32] [--hidden 128] [--layers 2] [--batch 1024] [--widths 16 64]
                                    [--plies 24] [--out profiles/blokus_net_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"


def _cell_table(bb):
    """(cells int64 [21, 8, 5, 5]: the offset dy * 64 + dx + 4 * 65 of each covered cell from the anchor, count int64 [21, 8, 5]) read
    off the library: every placement stepped onto the centre of an empty board"""
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    ids = torch.arange(21 * 8 * 5, device=DEV)
    probe = BlokusBatch(ids.numel(), device=DEV)
    probe.step(((((ids // 40) * 400 + 210) * 8 + (ids // 5) % 8) * 5 + ids % 5).to(torch.int32))
    own = probe.board() == 1                                                       # [840, 20, 20]: row y, column x
    count = own.view(len(ids), -1).sum(dim=1)
    order = torch.argsort((~own.view(len(ids), -1)).to(torch.int8), dim=1, stable=True)[:, :5]
    cells = (order // 20 - 10) * 64 + (order % 20 - 10) + 4 * 65
    return cells.view(21, 8, 5, 5), count.view(21, 8, 5)


def _torch_net(bb, hidden, layers):
    """the contract's network as a torch module: (module, its evaluator for puct)"""
    import torch
    cells, count = _cell_table(bb)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            body, n_in = [], bb.NET_FEATURES
            for _ in range(layers):
                body += [torch.nn.Linear(n_in, hidden), torch.nn.ReLU()]
                n_in = hidden
            self.body = torch.nn.Sequential(*body)
            self.cells, self.pieces, self.value = torch.nn.Linear(hidden, 400), torch.nn.Linear(hidden, 21), torch.nn.Linear(hidden, 4)

        def forward(self, board, pieces, cand, n_cand, mover):
            b = board.view(board.shape[0], 400)
            x = torch.cat([b == 0, b == 1, b == 2, b == 3, pieces.view(-1, 84) != 0], dim=1).float()
            h = self.body(x)
            q, r = self.cells(h), self.pieces(h)
            a = cand.to(torch.int64).clamp(0, 335999)
            piece, anchor, orient, shift = a // 16000, (a // 40) % 400, (a // 5) % 8, a % 5
            n = torch.where((cand >= 0) & (cand < 336000), count[piece, orient, shift], 0)
            off = cells[piece, orient, shift]                                      # [B, W, 5]
            X, Y = (anchor % 20).unsqueeze(2) + off % 64 - 4, (anchor // 20).unsqueeze(2) + off // 64 - 4
            on = (torch.arange(5, device=DEV) < n.unsqueeze(2)) & (X >= 0) & (X < 20) & (Y >= 0) & (Y < 20)
            m = (mover.to(torch.int64) & 3).view(-1, 1, 1)
            i = torch.where(m == 0, Y, torch.where(m == 1, X, torch.where(m == 2, 19 - Y, 19 - X)))
            j = torch.where(m == 0, X, torch.where(m == 1, 19 - Y, torch.where(m == 2, 19 - X, Y)))
            got = torch.gather(q, 1, (20 * i + j).clamp(0, 399).view(q.shape[0], -1)).view(on.shape)
            logit = torch.where(n > 0, torch.gather(r, 1, piece), 0.0) + (got * on).sum(dim=2)
            beyond = torch.arange(cand.shape[1], device=DEV) >= n_cand.clamp(0, cand.shape[1]).unsqueeze(1)
            return logit.masked_fill(beyond, float("-inf")), self.value(h)
    net = Net().to(DEV)

    def evaluate(leaves):
        with torch.no_grad():
            logit, value = net(leaves["board"], leaves["pieces"], leaves["cand"], leaves["n_cand"], leaves["mover"])
        return torch.softmax(logit, dim=1), torch.sigmoid(value)
    return net, evaluate


def _layers(net):
    linear = [m for m in net.body if hasattr(m, "weight")]
    return ([(m.weight, m.bias) for m in linear], (net.cells.weight, net.cells.bias), (net.pieces.weight, net.pieces.bias),
            (net.value.weight, net.value.bias))


def _simulations(bb, S, W, evaluate, leaves):
    """microseconds per simulation of S x (select, evaluate, backup) between two events, from a fresh search"""
    import torch
    bb.puct_begin(S, W, seed=3)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(S):
        bb.puct_select(1.25, 0.5, out=leaves)
        prior, value = evaluate(leaves)
        if prior.is_floating_point():
            prior, value = bb.puct_quantize(prior, value)
        bb.puct_backup(prior, value)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / S


def rows_of(widths, B, S, reps, hidden, layers, plies):
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    rows = []
    for W in widths:
        torch.manual_seed(0)
        bb = BlokusBatch(B, device=DEV)
        bb.rollout(plies, seed=7)                                                  # mid-game positions
        module, torch_eval = _torch_net(bb, hidden, layers)
        net = bb.net_pack(*_layers(module))
        const = (torch.ones((B, W), dtype=torch.int16, device=DEV), torch.full((B, 4), 32768, dtype=torch.int32, device=DEV))
        evaluators = {"torch": torch_eval, "hip": net.evaluator(), "const": lambda leaves: const}
        bb.puct_begin(S, W, seed=3)
        leaves = bb.puct_select(1.25, 0.5)
        times = {name: [] for name in evaluators}
        for rep in range(reps + 1):                                                # the first round is the warm-up of every launch
            for name, fn in evaluators.items():                                   # alternating: torch, hip, const, torch, ...
                t = _simulations(bb, S, W, fn, leaves)
                if rep:
                    times[name].append(t)
        out = bb.net_eval(net, leaves)
        eval_ms = M.median(M.back_to_back(lambda: bb.net_eval(net, leaves, out=out), S, reps, warmup=S))
        pack_ms = M.median(M.back_to_back(lambda: net.repack(*_layers(module)), S, reps, warmup=4))
        (t_med, t_rng), (h_med, h_rng), (c_med, _) = (M.spread(times[name]) for name in ("torch", "hip", "const"))
        row = {"game": "blokus", "B": B, "W": W, "S": S, "positions": "%d random plies from the reset" % plies,
               "network": {"inputs": bb.NET_FEATURES, "hidden": hidden, "layers": layers, "packed_bytes": int(net.packed.numel() * 8)},
               "reps": reps, "torch_sim_us": round(t_med, 2), "torch_sim_range_us": [round(x, 2) for x in t_rng],
               "hip_sim_us": round(h_med, 2), "hip_sim_range_us": [round(x, 2) for x in h_rng],
               "torch_over_hip": round(t_med / h_med, 3), "hip_faster_beyond_spread": bool(h_rng[1] < t_rng[0]),
               "net_eval_us": round(eval_ms * 1e3, 2), "pair_us": round(c_med, 2), "pack_us": round(pack_ms * 1e3, 2)}
        M.emit(row)
        rows.append(row)
        del bb, net
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--simulations", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--plies", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blokus_net_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 32 trees, widths 4 and 8, 4 simulations, one repetition, hidden 32")
    args = ap.parse_args()
    M.require_gpu("blokus_net_rate.py")
    import torch
    torch.cuda.set_device(0)
    if args.tiny:
        rows = rows_of([4, 8], 32, 4, 1, 32, args.layers, 8)
    else:
        rows = rows_of(args.widths, args.batch, args.simulations, args.reps, args.hidden, args.layers, args.plies)
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
