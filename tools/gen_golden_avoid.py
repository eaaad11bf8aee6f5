"""Generate tests/golden/tron_avoid_*.npz: games played by the reference's OWN SimpleAvoidAgent.

The reference module envs/tron/rllib.py is loaded with two stubs -- ``gym`` (and ``gym.spaces``) and ``TronRender``
(rendering is out of scope) -- on top of oracle/ref_loader.py's import shells.  Its module-level ``random`` is then
replaced by an object whose ``random()`` and ``choice()`` answer from the Philox words of the agent's contract
(include/colosseum_hip.h, crl_tron_sample_avoid), so every decision below is made by the reference's code and the
reference's TronGridEnvironment (next_cell, state_to_observation, next_state) plays the games.

Record i of a file is one step of one game, for draw coordinates g = i (the record index) and c = the step within its
game; it holds the pre-step state, the three Philox words of every player, the actions the reference agent took (0 for
dead players) and the state next_state produced.  Integer arrays only.

    python tools/gen_golden_avoid.py [--out tests/golden] [--check]

``--check`` regenerates into memory and compares with the committed files (exit status 1 on any difference).
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import rng_ref, tron_ref  # noqa: E402

SEED = 0x5EED_A701
# (N, P, noise as num / den, games, step cap per game)
CONFIGS = [
    (15, 4, 1, 10, 6, 400),
    (15, 2, 0, 10, 3, 400),
    (19, 4, 0, 10, 4, 400),
    (19, 3, 1, 10, 4, 400),
    (20, 2, 10, 10, 4, 400),
    (20, 4, 1, 10, 3, 400),
    (40, 3, 1, 10, 2, 300),
    (40, 4, 0, 10, 1, 300),
]
ACTION_CODE = {"forward": 0, "right": 1, "left": -1}


def file_name(N, P, num, den):
    return "tron_avoid_n%dp%d_z%d.npz" % (N, P, round(100 * num / den))


class ContractRandom:
    """Stands in for the reference module's ``random``: answers from the current player's Philox words."""

    def __init__(self):
        self.w = None
        self.noise = 0.0
        self.thr = 0

    def random(self):
        w0 = int(self.w[0])
        if w0 < self.thr:                       # noisy: a value <= noise
            return w0 / 4294967296.0
        return max(w0 / 4294967296.0, float(np.nextafter(self.noise, 2.0)))   # not noisy: a value > noise

    def choice(self, seq):
        if len(seq) == 3:
            return seq[(int(self.w[1]) * 3) >> 32]
        assert len(seq) == 2
        return seq[int(self.w[2]) >> 31]


def load_reference_agent():
    """The reference's envs/tron/rllib.py module with gym and TronRender stubbed."""
    from oracle import ref_loader
    ref = ref_loader.load()
    if "gym" not in sys.modules:
        gym = types.ModuleType("gym")
        spaces = types.ModuleType("gym.spaces")

        class _Space:
            def __init__(self, *a, **k):
                pass

        spaces.Dict = spaces.Discrete = spaces.Box = _Space
        gym.spaces = spaces
        gym.Env = object
        sys.modules["gym"] = gym
        sys.modules["gym.spaces"] = spaces
    render = types.ModuleType("colosseumrl.envs.tron.TronRender")

    class TronRender:
        def __init__(self, *a, **k):
            pass

    render.TronRender = TronRender
    sys.modules["colosseumrl.envs.tron.TronRender"] = render
    if not hasattr(np, "infty"):                # (numpy 2 dropped the alias the module's observation_space uses)
        np.infty = np.inf
    mod = importlib.import_module("colosseumrl.envs.tron.rllib")
    return ref, mod


def play(ref, mod, N, P, noise, games, cap, seed=SEED):
    fake = ContractRandom()
    fake.noise = noise
    fake.thr = rng_ref.threshold(noise)
    mod.random = fake
    agent = mod.SimpleAvoidAgent(noise=noise)
    env = ref["tron"].create(board_size=N, num_players=P)
    rec = {k: [] for k in ("c", "board", "heads", "dirs", "deaths", "words", "actions",
                           "next_board", "next_heads", "next_dirs", "next_deaths")}
    for _ in range(games):
        state, players = env.new_state(spawn_offset=2)
        for c in range(cap):
            board, heads, dirs, deaths = state
            g = len(rec["c"])
            w = np.stack(tron_ref.words(np.uint64(g), np.uint64(c), np.arange(P, dtype=np.uint64), seed), axis=1)
            acts = np.zeros(P, np.int8)
            names = []
            for p in players:
                fake.w = w[p]
                names.append(agent(env, env.state_to_observation(state, p)))
                acts[p] = ACTION_CODE[names[-1]]
            state, players, _, terminal, _ = env.next_state(state, players, names)
            nb, nh, nd, nk = state
            rec["c"].append(c)
            rec["board"].append(board.ravel().astype(np.int8))
            rec["heads"].append(heads.astype(np.int16))
            rec["dirs"].append(dirs.astype(np.int8))
            rec["deaths"].append(deaths.astype(np.int8))
            rec["words"].append(w.astype(np.uint32))
            rec["actions"].append(acts)
            rec["next_board"].append(nb.ravel().astype(np.int8))
            rec["next_heads"].append(nh.astype(np.int16))
            rec["next_dirs"].append(nd.astype(np.int8))
            rec["next_deaths"].append(nk.astype(np.int8))
            if terminal:
                break
    out = {k: np.stack(v) for k, v in rec.items()}
    out["c"] = out["c"].astype(np.uint32)
    return out


def situations(N, rec):
    """How many alive (record, player) decisions had the head against a wall ahead, and how many were boxed in (ahead
    and both sides occupied on the clamped probes)."""
    heads, dirs, deaths, board = rec["heads"].T, rec["dirs"].T, rec["deaths"].T, rec["board"]
    rows = np.arange(board.shape[0])[None, :]
    cell = lambda off: tron_ref.clamped_cell(N, heads, dirs.astype(np.int64) + off)
    alive = deaths == 0
    wall = alive & (cell(0) == heads)
    boxed = alive & (board[rows, cell(0)] != 0) & (board[rows, cell(1)] != 0) & (board[rows, cell(3)] != 0)
    return int(wall.sum()), int(boxed.sum())


def generate():
    ref, mod = load_reference_agent()
    files = {}
    for N, P, num, den, games, cap in CONFIGS:
        rec = play(ref, mod, N, P, num / den, games, cap)
        wall, boxed = situations(N, rec)
        rec.update(N=np.int64(N), P=np.int64(P), noise_num=np.int64(num), noise_den=np.int64(den), seed=np.int64(SEED),
                   n_wall=np.int64(wall), n_boxed=np.int64(boxed))
        files[file_name(N, P, num, den)] = rec
    return files


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    files = generate()
    bad = 0
    for name, rec in files.items():
        path = os.path.join(args.out, name)
        if args.check:
            with np.load(path) as z:
                same = set(z.files) == set(rec) and all(np.array_equal(z[k], rec[k]) and z[k].dtype == rec[k].dtype for k in rec)
            bad += not same
            print("%-28s %s" % (name, "same" if same else "DIFFERS"))
        else:
            np.savez_compressed(path, **rec)
            print("%-28s %5d records  wall-ahead %4d  boxed-in %4d  %7d bytes" % (
                name, len(rec["c"]), int(rec["n_wall"]), int(rec["n_boxed"]), os.path.getsize(path)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
