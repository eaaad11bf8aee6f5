"""Times batched random playouts (TTTBatch / BlokusBatch.playout: crl_*_playout, one launch) against the random-agent
rollout (crl_*_rollout) at the same number of concurrent games.

Per configuration, device-event time of one playout call (median of --reps after a warm-up), and from its outputs
  * playouts_per_s, plies_per_s (len_sum over all rows: every ply played, candidate plies included)
  * rollout_env_steps_per_s: crl_*_rollout on as many games as the call runs playouts at once (capped at 2^24 games for
    TicTacToe), --roll-steps plies per game
  * plies_over_rollout: the ratio of the two rates
  * TicTacToe only, lane_efficiency: useful lane-plies over issued ones -- sum of plies / (64 x sum over waves of the
    wave's longest playout) -- of R = 1 playouts from the same positions (i.i.d. lengths, as the R lanes of a row are), the
    fraction of a wave's lanes doing work while the wave runs to its longest playout.  Blokus runs one wave per playout.
TicTacToe: 3x3 P2, 3x5 P3, 3x3x3 P4, 5x5 K4 P3 from the empty board (cand = NULL) at 2^24 and 2^28 playouts.  Blokus:
1,024 positions (16 random plies in) x 16 candidates (random legal ids by select on random ranks) x 16 playouts, and
16,384 x 1 x 1 from the initial position.  Prints one JSON line per configuration and writes them to --out.

    python tools/playout_rate.py [--reps 3] [--out profiles/playout_rate.jsonl] [--tiny]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"


def _lane_efficiency(make, n):
    """useful over issued lane-plies of n R = 1 playouts, 64 consecutive ones per wave"""
    b = make(n)
    lens = b.playout(1)["len_sum"].view(-1, 64).to(torch.float64)
    return float(lens.sum() / (64.0 * lens.max(dim=1).values.sum()))


def ttt_rows(shapes, sizes, reps, roll_steps, roll_cap):
    from colosseumrl_amd.batched import TTTBatch
    rows = []
    for dims, k, p in shapes:
        name = M.shape_name(dims, k, p)
        eff = _lane_efficiency(lambda n: TTTBatch(dims, k, p, n, device=DEV), 1 << 16)
        for log2 in sizes:
            B = 1 << 14 if log2 > 16 else 1 << (log2 // 2)
            R = (1 << log2) // B
            tb = TTTBatch(dims, k, p, B, device=DEV)
            out = tb.playout(R)
            ms = M.median(M.isolated(lambda: tb.playout(R, out=out), reps, warmup=1))
            plies = int(out["len_sum"].to(torch.int64).sum())
            n_roll = min(B * R, roll_cap)
            roll = TTTBatch(dims, k, p, n_roll, device=DEV)
            ms_roll = M.median(M.isolated(lambda: roll.rollout(roll_steps), reps, warmup=1))
            row = {"game": "tictactoe", "shape": name, "B": B, "A": 1, "R": R, "playouts": B * R, "ms": round(ms, 3),
                   "playouts_per_s": round(B * R / ms * 1e3), "plies_per_s": round(plies / ms * 1e3),
                   "mean_plies": round(plies / (B * R), 3),
                   "rollout_games": n_roll, "rollout_env_steps_per_s": round(n_roll * roll_steps / ms_roll * 1e3),
                   "lane_efficiency": round(eff, 4)}
            row["plies_over_rollout"] = round(row["plies_per_s"] / row["rollout_env_steps_per_s"], 3)
            M.emit(row)
            rows.append(row)
            del tb, roll, out
            torch.cuda.empty_cache()
    return rows


def blokus_rows(configs, reps, roll_steps):
    from colosseumrl_amd.batched import BlokusBatch
    rows = []
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    for B, A, R, warm in configs:
        bb = BlokusBatch(B, device=DEV)
        cand = None
        if warm:
            bb.rollout(warm, seed=1)                        # positions `warm` random plies in (no game ends that early)
            bb.tcount.zero_()
            _, count = bb.select(torch.zeros(B, dtype=torch.int32, device=DEV))
            cols = []
            for _ in range(A):
                rank = (torch.randint(0, 1 << 30, (B,), generator=gen, device=DEV) % count.clamp(min=1)).to(torch.int32)
                cols.append(bb.select(rank)[0])
            cand = torch.stack(cols, dim=1).contiguous()
        out = bb.playout(R, cand)
        ms = M.median(M.isolated(lambda: bb.playout(R, cand, out=out), reps, warmup=1))
        plies = int(out["len_sum"].to(torch.int64).sum())
        n = B * A * R
        roll = BlokusBatch(n, device=DEV)
        ms_roll = M.median(M.isolated(lambda: roll.rollout(roll_steps), reps, warmup=1))
        row = {"game": "blokus", "B": B, "A": A, "R": R, "playouts": n, "start_plies": warm, "ms": round(ms, 3),
               "playouts_per_s": round(n / ms * 1e3), "plies_per_s": round(plies / ms * 1e3),
               "mean_plies": round(plies / n, 2), "rollout_games": n,
               "rollout_env_steps_per_s": round(n * roll_steps / ms_roll * 1e3),
               "rollout_us_per_ply": round(ms_roll * 1e3 / roll_steps, 2),
               "playout_us_per_mean_ply": round(ms * 1e3 / (plies / n), 2)}
        row["plies_over_rollout"] = round(row["plies_per_s"] / row["rollout_env_steps_per_s"], 3)
        M.emit(row)
        rows.append(row)
        del bb, roll, out
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a few thousand playouts per configuration (a smoke run)")
    args = ap.parse_args()
    M.require_gpu("playout_rate.py")
    torch.cuda.set_device(0)
    if args.tiny:
        rows = ttt_rows(M.TTT_SHAPES[:1], [12], 1, 8, 1 << 12) + blokus_rows([(8, 2, 2, 16), (16, 1, 1, 0)], 1, 4)
    else:
        rows = (ttt_rows(M.TTT_SHAPES, [24, 28], args.reps, 16, 1 << 24)
                + blokus_rows([(1024, 16, 16, 16), (16384, 1, 1, 0)], args.reps, 16))
    M.write_rows(args.out, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
