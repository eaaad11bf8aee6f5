"""Times TicTacToe's tactical (win-or-block) agent next to the random agent it stands beside, and the same figures of a
PARENT build of the library next to both, so that a change is held to the code before it and not to itself.  A parent that
exports the tactical entries is measured with both agents; one from before them with the random agent alone.

Per shape (3x3 P2, 3x5 K3 P3, 3x3x3 P4, 5x5 K4 P3) at B = 262,144 games, --noise 0.1, device-event times after a warm-up:
  * step_single_us    us per step_single call (one learner step, the opponents' plies included; the learner plays a uniform
                      cell drawn beforehand, an occupied one passes), over --steps calls from a reset batch
  * playout_plies_per_s   plies/s of one playout call, 2^28 playouts (16,384 positions x 16,384) from the empty board
  * rollout_env_steps_per_s   env-steps/s of rollout / rollout_tactical, --roll-steps plies per game
  * winning_cells_us  us per winning_cells call (this build only)
each for agent = random and tactical on this build and on the parent build (--parent-lib; tactical: if it has the entries;
winning_cells_us_parent likewise).  A library is
loaded once per process, so every measurement round is a child process of its own -- this build, the parent, this build, ...
(--rounds of each, alternating) -- and a row reports per figure the median over the rounds and [min, max] as its spread.
Without --parent-lib the parent figures are null.  The parent build is the library of the commit before, e.g.
    git archive <commit> colosseumrl_amd/csrc include | tar -x -C build/parent_src && make -C build/parent_src/colosseumrl_amd/csrc
which leaves build/parent_src/colosseumrl_amd/libcolosseum_hip.so.  Prints one JSON line per shape and writes them to --out.

    python tools/tactical_rate.py [--rounds 3] [--noise 0.1] [--parent-lib PATH] [--out profiles/tactical_rate.jsonl] [--tiny]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.common import measure as M  # noqa: E402

DEV = "cuda:0"
SHAPES = M.TTT_SHAPES
TACTICAL_ENTRIES = ("crl_ttt_winning_cells", "crl_ttt_sample_tactical", "crl_ttt_rollout_tactical",
                    "crl_ttt_step_single_tactical", "crl_ttt_playout_tactical")
FIGURES = ("step_single_us", "playout_plies_per_s", "rollout_env_steps_per_s")


# ------------------------------------------------------------------ one round, in a process of its own
def _exports(lib_path, names):
    """whether the library exports every one of the entries"""
    import ctypes
    lib = ctypes.CDLL(lib_path)
    return all(hasattr(lib, name) for name in names)


def child(a):
    """one round: {shape: {figure_agent: value}} as a JSON line behind "ROUND "; a child that is given a library is the
    parent's"""
    import torch
    from colosseumrl_amd import _native
    tactical = not os.environ.get("CRL_LIB_PATH") or _exports(_native.LIB_PATH, TACTICAL_ENTRIES)
    agents = ["random", "tactical"] if tactical else ["random"]
    if not tactical:                                        # a build from before the tactical entries exports none of them
        for name in TACTICAL_ENTRIES:
            _native.PROTOTYPES.pop(name)
    from colosseumrl_amd.batched import TTTBatch
    M.require_gpu("tactical_rate.py")
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    out = {}
    for dims, k, p in SHAPES[:a.shapes]:
        row = {}
        tb = TTTBatch(dims, k, p, a.batch, device=DEV)
        seat = torch.zeros((a.batch,), dtype=torch.int8, device=DEV)
        acts = [torch.randint(0, tb.n_cells, (a.batch,), generator=gen, device=DEV) for _ in range(a.steps)]
        pb = TTTBatch(dims, k, p, a.playout_batch, device=DEV)
        R = a.playouts // a.playout_batch
        for agent in agents:
            kw_single = {"opponent": agent, "noise": a.noise} if tactical else {}
            kw_playout = {"agent": agent, "noise": a.noise} if tactical else {}
            bufs = {}

            def run_single():
                for i in range(a.steps):
                    bufs["s"] = tb.step_single(seat, acts[i], 3, out=bufs.get("s"), **kw_single)
            tb.reset()
            tb.step_single(seat, None, 3, **kw_single)
            row["step_single_us_" + agent] = M.median(M.isolated(run_single, a.reps, warmup=1)) * 1e3 / a.steps
            po = pb.playout(R, **kw_playout)
            ms = M.median(M.isolated(lambda: pb.playout(R, out=po, **kw_playout), a.reps, warmup=1))
            row["playout_plies_per_s_" + agent] = int(po["len_sum"].to(torch.int64).sum()) / (ms * 1e-3)
            roll = (lambda: tb.rollout_tactical(a.roll_steps, 3, a.noise)) if agent == "tactical" else (lambda: tb.rollout(a.roll_steps, 3))
            tb.reset()
            row["rollout_env_steps_per_s_" + agent] = a.batch * a.roll_steps / (M.median(M.isolated(roll, a.reps, warmup=1)) * 1e-3)
        if tactical:
            row["winning_cells_us"] = M.median(M.isolated(tb.winning_cells, a.reps, warmup=1)) * 1e3     # (the positions the rollouts left)
        out[M.shape_name(dims, k, p)] = row
        del tb, pb
        torch.cuda.empty_cache()
    print("ROUND " + json.dumps(out), flush=True)


# ------------------------------------------------------------------ the rounds, alternating builds
def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--playouts", type=int, default=1 << 28)
    ap.add_argument("--playout-batch", type=int, default=1 << 14)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--roll-steps", type=int, default=2048)
    ap.add_argument("--noise", type=float, default=0.1, help="the tactical agent's noise (1 = every ply uniform: no winning-cell set)")
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="the first so many shapes")
    ap.add_argument("--parent-lib", default=None, help="libcolosseum_hip.so of the parent commit (see above)")
    ap.add_argument("--round-timeout", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tactical_rate.jsonl"))
    ap.add_argument("--tiny", action="store_true", help="a seconds-long smoke run (two shapes, 1,024 games, 2^12 playouts, one round)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.tiny:
        a.rounds, a.reps, a.batch, a.playouts, a.playout_batch, a.steps, a.roll_steps, a.shapes = 1, 1, 1024, 1 << 12, 64, 4, 8, 2
    if a.child:
        return child(a)
    if a.parent_lib and not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib %s does not exist" % a.parent_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch), "--playouts", str(a.playouts),
           "--playout-batch", str(a.playout_batch), "--steps", str(a.steps), "--roll-steps", str(a.roll_steps),
           "--reps", str(a.reps), "--shapes", str(a.shapes), "--noise", str(a.noise)]
    builds = [("this", None)] + ([("parent", a.parent_lib)] if a.parent_lib else [])
    here, parent = [], []
    for tag, result in M.alternate(cmd, builds, a.rounds, a.round_timeout, "ROUND ", cwd=ROOT):
        (parent if tag == "parent" else here).append(result)
    rows = []
    for dims, k, p in SHAPES[:a.shapes]:
        name = M.shape_name(dims, k, p)
        row = {"game": "tictactoe", "shape": name, "B": a.batch, "noise": a.noise, "playouts": a.playouts, "steps": a.steps,
               "roll_steps": a.roll_steps, "rounds": a.rounds}
        for fig in FIGURES:
            for agent in ("random", "tactical"):
                row[fig + "_" + agent], row[fig + "_" + agent + "_spread"] = M.spread([r[name][fig + "_" + agent] for r in here])
            row[fig + "_random_parent"], row[fig + "_random_parent_spread"] = \
                M.spread([r[name][fig + "_random"] for r in parent]) if parent else (None, None)
            if parent and fig + "_tactical" in parent[0][name]:         # (a parent with the tactical entries)
                row[fig + "_tactical_parent"], row[fig + "_tactical_parent_spread"] = \
                    M.spread([r[name][fig + "_tactical"] for r in parent])
        row["winning_cells_us"], row["winning_cells_us_spread"] = M.spread([r[name]["winning_cells_us"] for r in here])
        if parent and "winning_cells_us" in parent[0][name]:
            row["winning_cells_us_parent"], row["winning_cells_us_parent_spread"] = \
                M.spread([r[name]["winning_cells_us"] for r in parent])
        row["step_single_tactical_over_random"] = row["step_single_us_tactical"] / row["step_single_us_random"]
        row["playout_random_over_tactical"] = row["playout_plies_per_s_random"] / row["playout_plies_per_s_tactical"]
        row["rollout_random_over_tactical"] = row["rollout_env_steps_per_s_random"] / row["rollout_env_steps_per_s_tactical"]
        row = {k_: (round(v, 3) if isinstance(v, float) else [round(x, 3) for x in v] if isinstance(v, list) else v)
               for k_, v in row.items()}
        M.emit(row)
        rows.append(row)
    M.write_rows(a.out, rows)


if __name__ == "__main__":
    main()
