"""Generate tests/golden/live_*.npz: the reference's answers to the seeded games of tests/test_reference_live.py.

TEST INFRASTRUCTURE.  Run as ``python -m oracle.gen_golden_live`` from the repository root where the reference
exists (see oracle/ref_loader.py).  The games are the ones those tests used to play against the reference itself:
the same seeds, the same random agents, the same lengths.  Every action and every reference output the tests compare
the oracle with is stored, so the tests replay the games through the oracle without the reference.  Integers only,
plus (``live_blokus_wire``) the reference's own dill pickle of one Blokus state as bytes.
"""
import io
import os
import pickle
import sys

import numpy as np

from . import oracle as O
from . import ref_loader
from .gen_golden import OUT, TRON_ACT, TRON_ACT_INT, _winmask

TRON_CASES = [(8, 2), (11, 3), (20, 4), (16, 5), (23, 7), (12, 8), (40, 4)]
TTT_CASES = [("ttt2", (3, 3), 2), ("ttt3", (3, 5), 3), ("ttt4", (3, 3, 3), 4)]


def tron_games(R, N, P, games=25, steps=60):
    rng = np.random.default_rng(N * 100 + P)
    env = R["tron"]("%d;%d" % (N, P))
    rec = {k: [] for k in ("start_heads", "start_dirs", "game_len", "actions", "board", "heads", "dirs", "deaths", "rewards",
                           "terminal", "winmask", "observer", "obs_board", "obs_heads", "ranking")}
    for game in range(games):
        s, _ = env.new_state()
        rec["start_heads"].append(s[1].copy())
        rec["start_dirs"].append(s[2].copy())
        n = 0
        for t in range(steps):
            a = rng.integers(0, 3, size=P)
            s, pl, rew, term, win = env.next_state(s, list(range(P)), [TRON_ACT[i] for i in a])
            rec["actions"].append(TRON_ACT_INT[a])
            rec["board"].append(s[0].reshape(-1).copy())
            for k, v in (("heads", s[1]), ("dirs", s[2]), ("deaths", s[3]), ("rewards", rew)):
                rec[k].append(np.array(v).copy())
            rec["terminal"].append(bool(term))
            rec["winmask"].append(_winmask(win))
            n += 1
            if term and t > 5 + game:
                break
        rec["game_len"].append(n)
        obs = env.state_to_observation(s, game % P)
        rec["observer"].append(game % P)
        rec["obs_board"].append(obs["board"].reshape(-1).copy())
        rec["obs_heads"].append(np.array(obs["heads"]).copy())
        rk = env.compute_ranking(s, list(range(P)), [] if win is None else list(win))
        rec["ranking"].append([rk[p] for p in range(P)])
    types = dict(start_heads=np.int16, start_dirs=np.int8, game_len=np.int32, actions=np.int8, board=np.int8, heads=np.int16,
                 dirs=np.int8, deaths=np.int8, rewards=np.int8, terminal=np.uint8, winmask=np.uint8, observer=np.int8,
                 obs_board=np.int8, obs_heads=np.int16, ranking=np.int8)
    return {k: _exact(rec[k], types[k]) for k in rec}


def ttt_games(R, which, dims, P, games=40):
    rng = np.random.default_rng(P)
    env = R[which]()
    n_cells = int(np.prod(dims))
    rec = {k: [] for k in ("game_len", "cell", "board", "winner", "to_move", "reward", "terminal", "win")}
    for game in range(games):
        s, pl = env.new_state()
        for t in range(n_cells + 4):
            cell = int(rng.integers(-1, n_cells))
            astr = "" if cell < 0 else str(tuple(int(i) for i in np.unravel_index(cell, dims)))
            s, pl, rew, term, win = env.next_state(s, pl, [astr])
            rec["cell"].append(cell)
            rec["board"].append(s[0].ravel().copy())
            rec["winner"].append(-1 if s[1] is None else s[1])
            rec["to_move"].append(pl[0])
            rec["reward"].append(rew[0])
            rec["terminal"].append(bool(term))
            rec["win"].append(-1 if win is None else win[0])
        rec["game_len"].append(n_cells + 4)
    types = dict(game_len=np.int32, cell=np.int8, board=np.int8, winner=np.int8, to_move=np.int8, reward=np.int8,
                 terminal=np.uint8, win=np.int8)
    return {k: _exact(rec[k], types[k]) for k in rec}


def blokus_games(R, games=2, plies=12):
    env = R["blokus"]()
    rng = np.random.default_rng(2024)
    rec = {k: [] for k in ("valid_count", "valid_ids", "action", "board", "score", "reward", "terminal", "to_move", "round")}
    for game in range(games):
        s, pl = env.new_state()
        for t in range(plies):
            va = env.valid_actions(s, pl[0])
            ids_ref = [O.blokus_action_id(a) for a in va if a]
            a = ids_ref[int(rng.integers(0, len(ids_ref)))] if ids_ref else -1
            s, pl, rew, term, win = env.next_state(s, pl, [O.blokus_action_string(a)])
            rec["valid_count"].append(len(ids_ref))
            rec["valid_ids"].extend(ids_ref)
            rec["action"].append(a)
            rec["board"].append(np.array(s[0].board_contents).copy())
            rec["score"].append([p.player_score for p in s[2]])
            rec["reward"].append(rew[0])
            rec["terminal"].append(bool(term))
            rec["to_move"].append(pl[0])
            rec["round"].append(s[1])
    types = dict(valid_count=np.int32, valid_ids=np.int32, action=np.int32, board=np.int8, score=np.int32, reward=np.int32,
                 terminal=np.uint8, to_move=np.int8, round=np.int32)
    out = {k: _exact(rec[k], types[k]) for k in rec}
    out["plies"] = np.array([plies] * games, np.int32)
    return out


def blokus_wire(R):
    """The reference's own pickle of a state two plies in, its data members, the class paths the pickle names and the
    reference's valid_actions on it (as action ids)."""
    env = R["blokus"]()
    s, pl = env.new_state()
    for a in ("monomino1;(0, 0);north0", "domino1;(19, 0);south0"):
        s, pl, *_ = env.next_state(s, pl, [a])
    data = env.serialize_state(s)
    return {"pickle": np.frombuffer(bytes(data), np.uint8).copy(),
            "board": _exact(s[0].board_contents, np.int8), "round": np.array(s[1], np.int32), "to_move": np.array(pl[0], np.int8),
            "score": _exact([p.player_score for p in s[2]], np.int32), "color": _exact([p.player_color for p in s[2]], np.int32),
            "pieces": np.array([";".join(p.current_pieces) for p in s[2]]),
            "classes": np.array(sorted(c for c in _classes(data) if c.startswith("colosseumrl."))),
            "valid_ids": _exact([O.blokus_action_id(a) for a in env.valid_actions(s, pl[0]) if a], np.int32)}


def _classes(data):
    """Every "module.name" the pickle asks its loader for."""
    seen = set()

    class Recorder(pickle.Unpickler):
        def find_class(self, module, name):
            seen.add(module + "." + name)
            return super().find_class(module, name)
    Recorder(io.BytesIO(bytes(data))).load()
    return seen


def _exact(values, dtype):
    a = np.asarray(values)
    b = a.astype(dtype)
    assert np.array_equal(a, b), "values do not fit %s" % np.dtype(dtype).name
    return b


def main(argv):
    R = ref_loader.load()
    what = argv or ["tron", "ttt", "blokus"]
    if "tron" in what:
        for N, P in TRON_CASES:
            np.savez_compressed(os.path.join(OUT, "live_tron_n%dp%d.npz" % (N, P)), **tron_games(R, N, P))
    if "ttt" in what:
        for which, dims, P in TTT_CASES:
            np.savez_compressed(os.path.join(OUT, "live_%s.npz" % which), dims=np.array(dims, np.int32), **ttt_games(R, which, dims, P))
    if "blokus" in what:
        np.savez_compressed(os.path.join(OUT, "live_blokus.npz"), **blokus_games(R))
        np.savez_compressed(os.path.join(OUT, "live_blokus_wire.npz"), **blokus_wire(R))


if __name__ == "__main__":
    main(sys.argv[1:])
