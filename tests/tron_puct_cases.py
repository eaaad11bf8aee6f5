"""The case table of the crl_tron_puct_* tests: the shapes, the seeded positions, the seats and the edge rows.
tests/test_tron_puct_host.py runs every edge row on the restatement and requires that it reaches the edge it names;
tests/test_gpu_tron_puct.py runs the same rows on the GPU against the restatement."""
import functools

import numpy as np

from oracle import oracle as O
from tests import tron_mcts_ref as TM

# (N, P, model): trees that close within a few plies; 169 cells (planes off the 16-byte grid, a ragged tail); the headline
# board, whole chunks; the second Philox block of players 4..7 under both models; 1,089 bytes (more than one pass of 64 lanes
# x 16 B); one player (closed at depth 1)
SHAPES = [(5, 2, "random"), (13, 4, "avoid"), (20, 4, "random"), (9, 8, "random"), (9, 8, "avoid"), (33, 2, "avoid"), (5, 1, "random")]
SHAPE_IDS = ["5x5p2-random", "13x13p4-avoid", "20x20p4-random", "9x9p8-random", "9x9p8-avoid", "33x33p2-avoid", "5x5p1-random"]
BATCHES = (1, 5, 130)        # fewer trees than waves, a ragged last workgroup, more than one trip of a capped grid's stride
S_MAIN = 40
SEED, FIRST_ENV_ID, NOISE = 0x1234567887654321, (1 << 32) - 2, 0.25     # (g wraps inside the batch)


@functools.lru_cache(maxsize=None)
def state(N, P, B, seed=0):
    """An oracle state of B positions: even rows from tron_mcts_ref.positions (avoid-agent games after some steps, tcount with
    the counter wrap 2^32 - 3 in front), odd rows from late_positions (walled-up boards: terminal leaves at depth 1).  The
    callers never write it."""
    rng = np.random.default_rng([N * 31 + P, B, seed])
    a, b = TM.positions(N, P, B, rng), TM.late_positions(N, P, B, rng)
    odd = np.arange(B) % 2 == 1
    a.board[odd], a.heads[:, odd], a.dirs[:, odd], a.deaths[:, odd] = b.board[odd], b.heads[:, odd], b.dirs[:, odd], b.deaths[:, odd]
    # the counter wrap on even rows too (row 3, where `positions` puts it, is a walled-up board that closes within three plies):
    # row 0, which every B has, and row 4, so that `tcount + depth` passes 2^32 at depth 3 in open games of both models
    a.tcount[0] = np.uint32(2 ** 32 - 3)
    if B > 4:
        a.tcount[4] = np.uint32(2 ** 32 - 2)
    return a


def seats(P, B):
    """the seat of every row: the players in turn (late_positions keeps player 0's walk: odd rows sit there), with seats out of
    range (P, -1) among them; dead seats come with the positions"""
    s = np.arange(B) % P
    s[np.arange(B) % 2 == 1] = 0
    s[np.arange(B) % 11 == 6] = P
    s[np.arange(B) % 11 == 10] = -1
    return s.astype(np.int8)


def deep_state():
    """A path deeper than 64 nodes: 67x67, two players, the seat at cell 0 heading east along the top row, player 1 at cell
    66 * 67 heading east along the bottom row.  With the avoid model at noise 0, cpuct = 0, fpu = 0 and a constant value of
    65536 each simulation goes one ply deeper; the step off the board at depth 67 closes the tree."""
    N = 67
    st = O.TronState(N, 2, 1)
    st.heads[:, 0], st.dirs[:, 0] = [0, 66 * N], [1, 1]
    st.board[0, 0], st.board[0, 66 * N] = 1, 2
    return st


DEEP = {"S": 70, "cpuct": 0, "fpu": 0, "mode": "win", "agent": "avoid", "noise": 0.0, "closes_at": 67}

# the edges, one row each: S simulations on a tree of capacity S_cap (default S), `extra` select + backup pairs behind them,
# the evaluator's mode (tests/tron_puct_ref.evaluator), and what the restatement's count must show for the row to be worth
# its name (B = 8 positions of the row's shape)
EDGE_CASES = [
    {"id": "S_cap=1", "shape": 0, "S": 1, "extra": 2, "reaches": {"refused": 4}},
    {"id": "at-capacity", "shape": 1, "S": 12, "extra": 2, "reaches": {"refused": 8, "created": 8}},
    {"id": "cpuct=0", "shape": 0, "S": 30, "cpuct": 0, "reaches": {"created": 8, "terminal": 1}},
    {"id": "cpuct=65535", "shape": 1, "S": 30, "cpuct": 65535, "reaches": {"created": 8, "depth": 2}},
    {"id": "fpu=0", "shape": 2, "S": 30, "fpu": 0, "reaches": {"created": 8, "depth": 3}},
    {"id": "fpu=65536", "shape": 3, "S": 30, "fpu": 65536, "reaches": {"created": 8}},
    {"id": "zero-priors", "shape": 0, "S": 30, "mode": "zero", "reaches": {"zero_sum": 30}},
    {"id": "prior-65535-clamped", "shape": 4, "S": 30, "mode": "clamp", "reaches": {"clamped": 8}},
    {"id": "values-outside", "shape": 5, "S": 30, "mode": "wild", "reaches": {"created": 8}},
    {"id": "select-twice", "shape": 1, "S": 30, "twice": True, "reaches": {"created": 8, "terminal": 1}},
    {"id": "leaf-NULL", "shape": 2, "S": 30, "no_leaf": True, "reaches": {"created": 8}},
]


def edge_state(case):
    N, P, agent = SHAPES[case["shape"]]
    return state(N, P, 8), seats(P, 8), agent
