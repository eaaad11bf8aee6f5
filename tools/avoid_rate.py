"""Times the scripted avoid agent's fused rollout against its two-call loop and the random-agent gquad rollout.

At B games (default 65,536), P = 4, noise 0.1, for each board size and launch length T: device-event times of
  * fused   -- TronBatch.rollout_avoid(T)                          (crl_tron_rollout_avoid, one launch)
  * loop    -- T x (sample_avoid(advance); step(auto_reset))       (crl_tron_sample_avoid + crl_tron_step, 2T launches)
  * gquad   -- TronBatch.rollout(T, kernel="gquad"), random agents (crl_tron_rollout, the lane-per-player global kernel)
after one warm-up of each; plus the mean episode length of both agents over the fused runs, and a check that the fused
and the loop states are identical.  Prints one JSON line per shape and writes them all to --out.

    python tools/avoid_rate.py [--batch 65536] [--sizes 19,40] [--steps 20,1024] [--reps 3] [--out FILE]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402


def _min_median_us(fn, reps):
    ts = [ms * 1e3 for ms in M.isolated(fn, reps)]
    return min(ts), M.median(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--players", type=int, default=4)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--sizes", default="19,40")
    ap.add_argument("--steps", default="20,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from colosseumrl_amd.batched import TronBatch
    M.require_gpu("avoid_rate.py")
    torch.cuda.set_device(0)
    B, P, noise = args.batch, args.players, args.noise
    rows = []
    for N in [int(x) for x in args.sizes.split(",")]:
        for T in [int(x) for x in args.steps.split(",")]:
            fused, loop, rnd = (TronBatch(N, P, B, device="cuda:0") for _ in range(3))

            def run_loop():
                for _ in range(T):
                    loop.step(loop.sample_avoid(7, noise), auto_reset=True)

            # warm-up (code objects, first-touch), then identical starting points for the equality check
            fused.rollout_avoid(T, 7, noise)
            run_loop()
            rnd.rollout(T, 7, kernel="gquad")
            torch.cuda.synchronize()
            same = all(torch.equal(a, b) for a, b in zip((fused.board, fused.heads, fused.dirs, fused.deaths, fused.tcount),
                                                        (loop.board, loop.heads, loop.dirs, loop.deaths, loop.tcount)))
            t_fused = _min_median_us(lambda: fused.rollout_avoid(T, 7, noise), args.reps)
            t_loop = _min_median_us(run_loop, args.reps)
            t_rnd = _min_median_us(lambda: rnd.rollout(T, 7, kernel="gquad"), args.reps)
            torch.cuda.synchronize()
            # (the loop keeps no episode statistics -- crl_tron_step does not --, so state and step counter are compared)
            same = same and all(torch.equal(a, b) for a, b in zip((fused.board, fused.heads, fused.dirs, fused.deaths, fused.tcount),
                                                                 (loop.board, loop.heads, loop.dirs, loop.deaths, loop.tcount)))
            mean_len = lambda tb: tb.len_sum.double().sum().item() / max(1.0, tb.n_episodes.double().sum().item())
            row = {"N": N, "P": P, "B": B, "T": T, "noise": noise,
                   "fused_us": round(t_fused[1], 1), "loop_us": round(t_loop[1], 1), "gquad_random_us": round(t_rnd[1], 1),
                   "fused_us_min": round(t_fused[0], 1), "loop_us_min": round(t_loop[0], 1), "gquad_random_us_min": round(t_rnd[0], 1),
                   "fused_us_per_step": round(t_fused[1] / T, 3), "gquad_random_us_per_step": round(t_rnd[1] / T, 3),
                   "loop_over_fused": round(t_loop[1] / t_fused[1], 2), "fused_over_gquad_random": round(t_fused[1] / t_rnd[1], 2),
                   "mean_episode_len_avoid": round(mean_len(fused), 2), "mean_episode_len_random": round(mean_len(rnd), 2),
                   "fused_equals_loop": bool(same)}
            M.emit(row)
            rows.append(row)
            del fused, loop, rnd
            torch.cuda.empty_cache()
    if args.out:
        M.write_rows(args.out, rows)
    return 0 if all(r["fused_equals_loop"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
