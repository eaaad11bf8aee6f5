"""Times the Blokus search valued by the caller's network (BlokusBatch.puct_*: crl_blokus_puct_select / _backup, two launches
per simulation for the whole batch, the trees in HBM, W sampled candidates per node) and, in the same run and process, the
launch floor and the self-contained playout search beside it.

Per width W = 8 and 64 -- --batch trees (1,024) from positions after 32 random plies; S = --simulations (128); the constant
evaluator (equal priors, every value 32768: two tensors made once, no launch between select and backup) -- device-event time,
median of --reps after a warm-up:
  * select_us, backup_us: one whole search with an event around every launch, the time of each kind summed over the S
    simulations and divided by S (a launch's share of a growing tree, not the time of a launch on a fixed tree)
  * pair_us: S select + backup pairs back to back between two events, divided by S
  * puct_ms: the whole puct() -- begin, S pairs, root -- and simulations_per_s = B S / that
  * step_observe_us: BlokusBatch.step_observe on the same batch, back to back: the launch floor;
    pair_over_two_step_observe = pair_us / (2 step_observe_us)
  * mcts_ms: BlokusBatch.mcts(S, 1, width=8) on the same batch, the self-contained search (one playout per leaf, one launch)
  * mean_nodes, mean_depth_last, mean_legal_last: the node count of a tree, and the plies from the root to, and the legal
    actions at, the pending leaves of the last simulation
With --pick-ab LIB (another build of the library, e.g. blokus_puct.hip compiled with -DBLK_PUCT_SERIAL_PICK: the candidates of
a leaf by W blk_select walks instead of one enumeration pass) select_us and pair_us are taken first for both builds at
--ab-widths (1, 4, 8, 64), a child process per build and round, the builds alternating, and go out as one more row per width.
Prints one JSON line per row and writes them to --out.

    python tools/blokus_puct_rate.py [--reps 3] [--batch 1024] [--simulations 128] [--out profiles/blokus_puct_rate.jsonl] [--tiny]
                                     [--pick-ab LIB [--ab-tag serial] [--ab-widths 1,4,8,64] [--rounds 3]]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"
WIDTHS = (8, 64)
PLIES = 32


def _per_kind(bb, S, W, prior, value, leaves):
    """(select, backup) microseconds per simulation of one search: an event around every launch"""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * S + 1)]
    bb.puct_begin(S, W, 1)
    torch.cuda.synchronize()
    ev[0].record()
    for s in range(S):
        bb.puct_select(1.25, 0.5, out=leaves)
        ev[2 * s + 1].record()
        bb.puct_backup(prior, value)
        ev[2 * s + 2].record()
    torch.cuda.synchronize()
    sel = sum(ev[2 * s].elapsed_time(ev[2 * s + 1]) for s in range(S))
    bak = sum(ev[2 * s + 1].elapsed_time(ev[2 * s + 2]) for s in range(S))
    return sel * 1e3 / S, bak * 1e3 / S


def _pairs(bb, S, W, prior, value, leaves):
    import torch
    bb.puct_begin(S, W, 1)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(S):
        bb.puct_select(1.25, 0.5, out=leaves)
        bb.puct_backup(prior, value)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / S


def child(widths, B, S, reps, plies):
    """one build's {W: [select_us, pair_us, mean legal actions at the last leaves]} behind "ROUND " on stdout"""
    import json
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    torch.cuda.set_device(0)
    out = {}
    for W in widths:
        bb = BlokusBatch(B, device=DEV)
        bb.rollout(plies, seed=7)
        prior = torch.ones((B, W), dtype=torch.int16, device=DEV)
        value = torch.full((B, 4), 32768, dtype=torch.int32, device=DEV)
        bb.puct(lambda leaves: (prior, value), S, W, seed=1)
        leaves = bb.puct_select()
        sel = M.median([_per_kind(bb, S, W, prior, value, leaves)[0] for _ in range(reps + 1)][1:])
        pair = M.median([_pairs(bb, S, W, prior, value, leaves) for _ in range(reps + 1)][1:])
        live = leaves["pending"] != 0
        out[str(W)] = [sel, pair, float(leaves["n_legal"][live].float().mean())]
    print("ROUND " + json.dumps(out), flush=True)
    return 0


def pick_ab(a, B, S, plies):
    """the rows of the two pick forms: this build against the one at a.pick_ab"""
    widths = [int(w) for w in a.ab_widths.split(",")]
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--ab-widths", a.ab_widths, "--batch", str(B), "--simulations", str(S),
           "--reps", str(a.reps), "--plies", str(plies)]
    got = {"this": [], a.ab_tag: []}
    for tag, result in M.alternate(cmd, [("this", None), (a.ab_tag, a.pick_ab)], a.rounds, 600, "ROUND ", cwd=ROOT):
        got[tag].append(result)
    rows = []
    for W in widths:
        row = {"game": "blokus", "figure": "pick A/B", "B": B, "S": S, "W": W, "rounds": a.rounds, "reps": a.reps,
               "positions": "%d random plies from the empty board" % plies,
               "mean_legal_last": round(got["this"][0][str(W)][2], 1) if got["this"][0][str(W)][2] == got["this"][0][str(W)][2] else None}
        for tag, name in (("this", "this"), (a.ab_tag, a.ab_tag)):
            for i, fig in enumerate(("select_us", "pair_us")):
                med, span = M.spread([r[str(W)][i] for r in got[tag]])
                row["%s_%s" % (fig, name)], row["%s_%s_spread" % (fig, name)] = round(med, 2), [round(x, 2) for x in span]
        row["select_%s_over_this" % a.ab_tag] = round(row["select_us_" + a.ab_tag] / row["select_us_this"], 3)
        M.emit(row)
        rows.append(row)
    return rows


def rows_of(widths, B, S, reps, plies=PLIES):
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    rows = []
    for W in widths:
        bb = BlokusBatch(B, device=DEV)
        bb.rollout(plies, seed=7)                                                 # mid-game positions
        keep = {k: getattr(bb, k).clone() for k in ("occ", "inv", "score", "round", "to_move", "tcount")}
        prior = torch.ones((B, W), dtype=torch.int16, device=DEV)
        value = torch.full((B, 4), 32768, dtype=torch.int32, device=DEV)

        def evaluate(leaves):
            return prior, value
        root = bb.puct(evaluate, S, W, seed=1)                                    # the warm-up of every launch
        leaves = bb.puct_select()
        kinds = [_per_kind(bb, S, W, prior, value, leaves) for _ in range(reps + 1)][1:]
        pair = M.median([_pairs(bb, S, W, prior, value, leaves) for _ in range(reps + 1)][1:])
        live = leaves["pending"] != 0                                             # the last simulation's pending leaves
        depth = float(leaves["depth"][live].float().mean()) if bool(live.any()) else None
        legal = float(leaves["n_legal"][live].float().mean()) if bool(live.any()) else None
        puct_ms = M.median(M.isolated(lambda: bb.puct(evaluate, S, W, seed=1, out=root), reps, warmup=1))
        nodes = float(root["nodes"].float().mean())
        mo = bb.mcts(S, 1, None, 8, 1)
        mcts_ms = M.median(M.isolated(lambda: bb.mcts(S, 1, None, 8, 1, out=mo), reps, warmup=1))
        obs = bb.step_observe()
        for k, v in keep.items():                                                 # step_observe on the searched positions
            getattr(bb, k).copy_(v)
        step_ms = M.median(M.back_to_back(lambda: bb.step_observe(out=obs), S, reps, warmup=S))
        row = {"game": "blokus", "B": B, "S": S, "W": W, "positions": "%d random plies from the empty board" % plies,
               "evaluator": "constant (no launch)", "reps": reps, "pick": "one enumeration pass",
               "select_us": round(M.median([x[0] for x in kinds]), 2), "backup_us": round(M.median([x[1] for x in kinds]), 2),
               "pair_us": round(pair, 2), "puct_ms": round(puct_ms, 4), "simulations_per_s": round(B * S / puct_ms * 1e3),
               "mean_nodes": round(nodes, 1), "mean_depth_last": None if depth is None else round(depth, 2),
               "mean_legal_last": None if legal is None else round(legal, 1),
               "step_observe_us": round(step_ms * 1e3, 2), "pair_over_two_step_observe": round(pair / (2 * step_ms * 1e3), 3),
               "mcts_ms": round(mcts_ms, 4), "puct_over_mcts_time": round(puct_ms / mcts_ms, 3)}
        M.emit(row)
        rows.append(row)
        del bb
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blokus_puct_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a smoke run: 32 trees after 12 plies, 8 simulations, width 8")
    ap.add_argument("--pick-ab", default=None, metavar="LIB", help="another build of the library to compare select against")
    ap.add_argument("--ab-tag", default="serial")
    ap.add_argument("--ab-widths", default="1,4,8,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--plies", type=int, default=PLIES)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.tiny:
        args.batch, args.simulations, args.reps, args.plies, args.rounds, args.ab_widths = 32, 8, 1, 12, 1, "8"
    if args.child:
        return child([int(w) for w in args.ab_widths.split(",")], args.batch, args.simulations, args.reps, args.plies)
    if args.pick_ab and not os.path.exists(args.pick_ab):
        raise SystemExit("--pick-ab %s does not exist" % args.pick_ab)
    ab = pick_ab(args, args.batch, args.simulations, args.plies) if args.pick_ab else []    # (before this process opens the GPU)
    M.require_gpu("blokus_puct_rate.py")
    import torch
    torch.cuda.set_device(0)
    rows = rows_of((8,) if args.tiny else WIDTHS, args.batch, args.simulations, args.reps, args.plies)
    M.write_rows(args.out, rows + ab)
    return 0


if __name__ == "__main__":
    sys.exit(main())
