"""Times a whole network-valued Tron search two ways in one process, the two alternating: the three-launch loop (puct_select,
net_eval, puct_backup per simulation: TronBatch.puct's loop with net.evaluator()) and the one-launch search
(TronBatch.puct_search: crl_tron_puct_search), on the same packed network and from the same positions.

Per configuration -- 11x11 P4 with 512 trees (examples/tron_alphazero.py's size) and 20x20 P4 with 4,096 trees, or --size /
--players / --batch; trees from the reset position, the avoid model at noise 0.1; S = --simulations (64); an MLP of --layers
(2) hidden layers of width --hidden (128), weights N(0, 9 / fan_in), biases N(0, 1) -- device-event time from a fresh search
after a warm-up round:
  * loop_sim_us, fused_sim_us: the S simulations between two events, divided by S; the median of --reps repetitions and their
    [min, max] (loop_sim_range_us, fused_sim_range_us)
  * fused_faster_beyond_spread: the slowest fused repetition is faster than the fastest repetition of the loop
  * same_root: the two searches end in the same root visits (they are byte-identical by contract; tests hold them to it)
Prints one JSON line per configuration and writes them to --out.

    python tools/tron_search_rate.py [--reps 5] [--simulations 64] [--hidden 128] [--layers 2] [--size N --players P --batch B]
                                     [--out profiles/tron_puct_search_rate.jsonl] [--tiny]
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


def _network(tb, hidden, layers):
    """a packed network with weights N(0, 9 / fan_in) and biases N(0, 1)"""
    import torch
    dims = [(hidden, 4 * tb.N * tb.N + 4)] + [(hidden, hidden)] * (layers - 1) + [(3, hidden), (1, hidden)]
    pairs = [(torch.randn(d, device=DEV) * 3.0 / d[1] ** 0.5, torch.randn(d[0], device=DEV)) for d in dims]
    return tb.net_pack(pairs[:-2], pairs[-2], pairs[-1])


def _timed(tb, S, run):
    """microseconds per simulation of run() between two events, from a fresh search"""
    import torch
    tb.puct_begin(S, agent="avoid", noise=0.1)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    run()
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
        net = _network(tb, hidden, layers)
        evaluate, state = net.evaluator(), {}

        def loop():
            for _ in range(S):
                state["leaves"] = tb.puct_select(1.25, 0.5, out=state.get("leaves"))
                tb.puct_backup(*evaluate(state["leaves"]))
        ways = {"loop": loop, "fused": lambda: tb.puct_search(net, S, 1.25, 0.5)}
        times, visits = {name: [] for name in ways}, {}
        for rep in range(reps + 1):                                            # the first round is the warm-up of every launch
            for name, run in ways.items():                                    # alternating: loop, fused, loop, ...
                t = _timed(tb, S, run)
                visits[name] = tb.puct_root()["visits"].clone()
                if rep:
                    times[name].append(t)
        (l_med, l_rng), (f_med, f_rng) = M.spread(times["loop"]), M.spread(times["fused"])
        row = {"game": "tron", "shape": "%dx%d_p%d" % (N, N, p), "B": B, "S": S, "positions": "reset, avoid model, noise 0.1",
               "network": {"inputs": 4 * N * N + 4, "hidden": hidden, "layers": layers, "packed_bytes": int(net.packed.numel() * 8)},
               "reps": reps, "loop_sim_us": round(l_med, 2), "loop_sim_range_us": [round(x, 2) for x in l_rng],
               "fused_sim_us": round(f_med, 2), "fused_sim_range_us": [round(x, 2) for x in f_rng],
               "loop_over_fused": round(l_med / f_med, 3), "fused_faster_beyond_spread": bool(f_rng[1] < l_rng[0]),
               "same_root": bool(torch.equal(visits["loop"], visits["fused"]))}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tron_puct_search_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 7x7 P2, 64 trees, 8 simulations, one repetition, hidden 32")
    args = ap.parse_args()
    M.require_gpu("tron_search_rate.py")
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
