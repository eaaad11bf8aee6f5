"""The case table of the crl_ttt_puct_* tests: the shapes, the seeded positions and the edge rows.  tests/test_ttt_puct_host.py
runs every row on the restatement and requires that it reaches the edge it names; tests/test_gpu_ttt_puct.py runs the same
rows on the GPU against the restatement."""
import functools

import numpy as np

from oracle import oracle as O
from tests.mcts_ref import Game, _empty_cells

# 3x3; 3x5 with three players; 27 cells with 13 line directions; 5x5 K4; 32 cells with 8 players (lane and bit 31, the most players)
SHAPES = [((3, 3), 3, 2), ((3, 5), 3, 3), ((3, 3, 3), 3, 4), ((5, 5), 4, 3), ((4, 8), 3, 8)]
SHAPE_IDS = ["3x3p2", "3x5p3", "3x3x3p4", "5x5k4p3", "4x8k3p8"]
KINDS = ("empty", "plies2", "plies5", "left1", "left2", "left3", "finished", "bad_mover")


def simulations(dims):
    """S of the main comparison: 40 on the small boards, 80 on 27 and 32 cells"""
    return 80 if int(np.prod(dims)) >= 27 else 40


def _quiet_fill(game, rng, left=None, plies=None):
    """a running position after `plies` plies, or with `left` empty cells: the players move in turn to random cells that
    complete no line (a game in which every cell would is started again)"""
    while True:
        occ, tm = [0] * game.P, 0
        while True:
            empty = _empty_cells(game, occ)
            if (left is not None and len(empty) == left) or (plies is not None and game.n - len(empty) == plies):
                return occ, tm
            quiet = [c for c in empty if not game.step(list(occ), tm, c)[0]]
            if not quiet:
                break
            game.step(occ, tm, int(rng.choice(quiet)))
            tm = (tm + 1) % game.P


@functools.lru_cache(maxsize=None)
def positions(dims, K, P, B, seed=0):
    """An oracle state of B positions whose rows cycle through KINDS: the empty board, after 2 and 5 random plies, with 1, 2 and
    3 empty cells (terminal leaves at depth 1), a finished game (a recorded winner) and a mover out of range."""
    game = Game(dims, K, P)
    rng = np.random.default_rng([sum(dims) * 17 + P, B, seed])
    st = O.TTTState(dims, K, P, B)
    for b in range(B):
        kind = KINDS[b % len(KINDS)]
        if kind == "empty":
            occ, tm = [0] * P, 0
        elif kind.startswith("plies"):
            occ, tm = _quiet_fill(game, rng, plies=int(kind[5:]))
        elif kind.startswith("left"):
            occ, tm = _quiet_fill(game, rng, left=int(kind[4:]))
        else:
            occ, tm = _quiet_fill(game, rng, plies=3)
        st.occ[:, b], st.to_move[b], st.winner[b] = occ, tm, -1
        if kind == "finished":
            st.winner[b] = (tm + P - 1) % P
        if kind == "bad_mover":
            st.to_move[b] = P if (b // len(KINDS)) % 2 == 0 else -1
    return st


# the edges, one row each: S simulations on a tree of capacity S_cap (default S), `extra` select + backup pairs behind them,
# the evaluator's mode (tests/puct_ref.evaluator), and what the restatement's count must show for the row to be worth its name
EDGE_CASES = [
    {"id": "S_cap=1", "shape": 0, "S": 1, "extra": 2, "reaches": {"refused": 6}},
    {"id": "at-capacity", "shape": 1, "S": 12, "extra": 2, "reaches": {"refused": 12, "created": 8}},
    {"id": "cpuct=0", "shape": 0, "S": 30, "cpuct": 0, "reaches": {"created": 8, "terminal": 1}},
    {"id": "cpuct=65535", "shape": 1, "S": 30, "cpuct": 65535, "reaches": {"created": 8, "depth": 2}},
    {"id": "fpu=0", "shape": 0, "S": 30, "fpu": 0, "reaches": {"created": 8, "depth": 3}},
    {"id": "fpu=65536", "shape": 3, "S": 30, "fpu": 65536, "reaches": {"created": 8}},
    {"id": "zero-priors", "shape": 0, "S": 30, "mode": "zero", "reaches": {"zero_sum": 30}},
    {"id": "priors-on-occupied-cells", "shape": 1, "S": 30, "mode": "occupied", "reaches": {"zero_sum": 30}},
    {"id": "prior-65535-clamped", "shape": 2, "S": 30, "mode": "clamp", "reaches": {"clamped": 30}},
    {"id": "values-outside", "shape": 4, "S": 30, "mode": "wild", "reaches": {"created": 8}},
    {"id": "select-twice", "shape": 0, "S": 30, "twice": True, "reaches": {"created": 8, "terminal": 1}},
    {"id": "leaf_occ-NULL", "shape": 2, "S": 30, "no_leaf_occ": True, "reaches": {"created": 8}},
]


def edge_state(case):
    d, k, p = SHAPES[case["shape"]]
    return positions(d, k, p, 8)
