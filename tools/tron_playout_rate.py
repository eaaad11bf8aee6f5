"""Times batched Tron playouts (TronBatch.playout: crl_tron_playout, one launch) against the fused rollouts and against the
replicate-and-loop way of getting the same numbers without it.

Per agent (random, avoid with noise 0.1) and board (19x19, 40x40; P = 4), from 4,096 mid-game positions x 3 candidate
first actions x 64 playouts, device-event time of one call (median of --reps after a warm-up), and from its outputs
  * steps_per_s (len_sum over all rows: every step played) and playouts_per_s;
  * rollout_env_steps_per_s: crl_tron_rollout / crl_tron_rollout_avoid on as many games as the call runs playouts,
    --roll-steps steps each, and steps_over_rollout, the ratio of the two rates;
  * loop_ms: the replicate-and-loop way -- repeat_interleave of the state A * R times, then sample[_avoid] (with the
    candidate written into the seat's row at step 0) + step without reset until every copy is done (one host check
    every 8 steps) -- and speedup_over_loop = loop_ms / ms.
Prints one JSON line per configuration and writes them to --out.

    python tools/tron_playout_rate.py [--reps 3] [--out profiles/tron_playout_rate.jsonl] [--tiny]
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


def _positions(N, B, agent):
    from colosseumrl_amd.batched import TronBatch
    tb = TronBatch(N, 4, B, device=DEV)
    tb.reset()
    if agent == "avoid":
        tb.rollout_avoid(N, 7, 0.1)
    else:
        tb.rollout(N // 4, 7)
    torch.cuda.synchronize()
    return tb


def _loop(tb, cand, R, agent, noise, seed):
    """the replicate-and-loop way: A * R copies of every position, then sample + step (no reset) until all are done"""
    from colosseumrl_amd.batched import TronBatch
    B, A = tb.B, cand.shape[1]
    M = B * A * R
    cp = TronBatch(tb.N, tb.P, M, device=DEV)
    cp.board.copy_(tb.board.repeat_interleave(A * R, dim=0))
    for name in ("heads", "dirs", "deaths"):
        getattr(cp, name).copy_(getattr(tb, name).repeat_interleave(A * R, dim=1))
    first = cand.reshape(-1).repeat_interleave(R).to(torch.int8)
    first = torch.where(first == 2, torch.full_like(first, -1), first)
    done = torch.zeros(M, dtype=torch.bool, device=DEV)
    k = 0
    while True:
        act = cp.sample_avoid(seed, noise) if agent == "avoid" else cp.sample(seed)
        if k == 0:
            act[0] = first
        cp.step(act)
        done |= cp.terminal.bool()
        k += 1
        if k % 8 == 0 and bool(done.all()):
            break
    return k


def rows(N_list, B, A, R, reps, roll_steps):
    from colosseumrl_amd.batched import TronBatch
    out = []
    for agent in ("random", "avoid"):
        for N in N_list:
            tb = _positions(N, B, agent)
            cand = torch.arange(A, dtype=torch.int32, device=DEV).expand(B, A).contiguous()
            po = tb.playout(R, cand, 1, agent=agent)
            ms = M.median(M.isolated(lambda: tb.playout(R, cand, 1, agent=agent, out=po), reps, warmup=1))
            steps = int(po["len_sum"].sum().item())
            n_play = int(po["played"].sum().item())
            games = B * A * R
            rb = TronBatch(N, 4, games, device=DEV)
            if agent == "avoid":
                rms = M.median(M.isolated(lambda: rb.rollout_avoid(roll_steps, 3, 0.1), reps, warmup=1))
            else:
                rms = M.median(M.isolated(lambda: rb.rollout(roll_steps, 3), reps, warmup=1))
            del rb
            roll_rate = games * roll_steps / (rms * 1e-3)
            lms = M.median(M.isolated(lambda: _loop(tb, cand, R, agent, 0.1, 1), max(1, reps), warmup=1))
            row = {"agent": agent, "N": N, "P": 4, "B": B, "A": A, "R": R, "ms": round(ms, 4),
                   "playouts_per_s": n_play / (ms * 1e-3), "steps_per_s": steps / (ms * 1e-3),
                   "mean_len": steps / max(n_play, 1), "rollout_env_steps_per_s": roll_rate,
                   "steps_over_rollout": (steps / (ms * 1e-3)) / roll_rate, "loop_ms": round(lms, 3),
                   "speedup_over_loop": lms / ms}
            M.emit(row)
            out.append(row)
            del tb
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--roll-steps", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tron_playout_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a seconds-long smoke run (64 positions x 3 x 8, 19x19 only)")
    a = ap.parse_args()
    M.require_gpu("tron_playout_rate.py")
    if a.tiny:
        res = rows([19], 64, 3, 8, 1, 8)
    else:
        res = rows([19, 40], 4096, 3, 64, a.reps, a.roll_steps)
    M.write_rows(a.out, res)


if __name__ == "__main__":
    main()
