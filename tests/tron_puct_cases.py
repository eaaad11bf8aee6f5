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
# behind the first seven (appended: the ids above keep their meaning): the other four template instances, P = 3, 5, 6 and 7,
# under both models on boards off the 16-byte grid (49 and 81 cells) -- tp_relative4's division by a P that is no power of
# two, the second Philox block serving one, two and three of players 4..7, the seat rotation wrapping at such a P --, and
# the smallest board the start layout has, 4x4: rows of exactly one 16-byte chunk, which is whole only where the output row
# happens to be aligned
N_FIRST_SHAPES = len(SHAPES)
SHAPES += [(7, 3, "random"), (7, 3, "avoid"), (7, 5, "random"), (7, 5, "avoid"), (9, 6, "random"), (9, 6, "avoid"), (9, 7, "random"),
           (9, 7, "avoid"), (4, 2, "avoid"), (4, 3, "random")]
SHAPE_IDS += ["%dx%dp%d-%s" % (N, N, P, agent) for N, P, agent in SHAPES[N_FIRST_SHAPES:]]
# fewer trees than waves; a ragged last workgroup; 33 workgroups of four waves, the last one ragged (ONE trip of the
# grid-stride loop: the grid is capped at 2^20 workgroups, tests/test_gpu_large.py takes the second trip)
BATCHES = (1, 5, 130)
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


def shape_seats(shape, B):
    """the seats of a shape's rows: `seats` for the first seven shapes; for the later ones the even rows go through the
    players one by one (b // 2 mod P: `seats` gives an even row b mod P, which never reaches an odd player of an even P), so
    that at B = 130 every player is the seat of a live tree (tests/test_tron_puct_host.py requires it)"""
    N, P, agent = SHAPES[shape]
    s = seats(P, B)
    if shape >= N_FIRST_SHAPES:
        b = np.arange(B)
        turn = (b % 2 == 0) & (b % 11 != 6) & (b % 11 != 10)
        s[turn] = ((b // 2) % P)[turn]
    return s


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


# ---- boards of fewer than 16 cells (tp_stream_row's `head = min(NN, ...)` decides, no whole chunk): the start layout needs
# N >= 4, so these are laid by hand, 8 rows each with their own directions and step counters, S = 6
def tiny_states():
    """[(id, state, seat, agent, noise)]: 3x3 with two players -- the seat in a corner, player 1 in the opposite one, the
    directions turning from row to row; 2x2 with one player, whose every child is closed (a single player's game is over
    when it is dead, and only then), so that the root is the only pending leaf"""
    three = O.TronState(3, 2, 8)
    for b in range(8):
        h0, h1 = ((0, 8), (2, 6), (8, 0), (6, 2))[b % 4]
        three.heads[:, b], three.dirs[:, b] = [h0, h1], [b % 4, (b // 2 + 1) % 4]
        three.board[b, h0], three.board[b, h1] = 1, 2
        if b >= 4:                                               # a trail cell in the middle of an edge, next to the seat's corner
            three.board[b, (1, 5, 7, 3)[b % 4]] = 1
    three.tcount[:] = [0, 1, 6, 7, 8, 2 ** 32 - 1, 2 ** 31, 12345]
    two = O.TronState(2, 1, 8)
    for b in range(8):
        two.heads[0, b], two.dirs[0, b] = b % 4, (b // 2) % 4
        two.board[b, b % 4] = 1
        if b >= 4:
            two.board[b, (b + 2) % 4] = 1                        # the diagonal cell taken: it is never probed
    two.tcount[:] = [3, 2 ** 32 - 1, 0, 9, 10, 11, 2 ** 31, 77]
    return [("3x3p2-avoid", three, (np.arange(8) % 2 * (np.arange(8) >= 4)).astype(np.int8), "avoid", NOISE),
            ("2x2p1-random", two, np.zeros(8, np.int8), "random", NOISE)]


TINY_S = 6


# ---- the workgroup shapes of `select`: four waves up to 127x127, three for 128..147, two for 148..180, one at 181
LDS_CASES = [(127, 2, 5), (128, 2, 5), (147, 2, 5), (148, 2, 5), (180, 2, 5), (181, 2, 5), (181, 8, 3)]
LDS_IDS = ["%dx%dp%d-B%d" % (N, N, P, B) for N, P, B in LDS_CASES]
LDS_S = 12


@functools.lru_cache(maxsize=None)
def lds_state(N, P, B):
    """(state, seat): avoid-agent games after at most 30 steps (the defaults play N*N / P oracle steps: seconds per board).
    On the 181x181 board, row 0 has the seat's head in the last cell (32,760: the last row and the last column, forward and
    right leave the board) and row 1 has player 1's head in the last row at cell 32,730, the top of what an int16 head and
    umulhi(h, inv_n) have to carry.  The callers never write it."""
    st = TM.positions(N, P, B, np.random.default_rng([N, P, B]), most=30)
    seat = (np.arange(B) % P).astype(np.int8)
    if N == 181:
        for b, p, cell, d in ((0, 0, N * N - 1, 1), (1, 1, 180 * N + 150, 1)):
            assert st.board[b, cell] == 0 and st.deaths[p, b] == 0 and seat[b] == p
            st.board[b, cell], st.heads[p, b], st.dirs[p, b] = p + 1, cell, d     # (the old head stays behind as trail)
    return st, seat


# ---- a tree at the greatest capacity: 20x20, two players, the start layout, the avoid model at noise 0 (with the table's
# noise the seat finds a line in which the other player kills itself within four plies, and the tree stays at 80 nodes), the
# rows told apart by their step counters.  Second: the exploration term at the top of its range while n grows.
CAPACITY = [{"id": "S=4095", "S": 4095, "cpuct": 256, "reaches": {"nodes": 2049, "depth": 12, "n": 256, "w": 1 << 26}},
            {"id": "cpuct=65535", "S": 1024, "cpuct": 65535, "reaches": {"nodes": 257, "depth": 8, "n": 256}}]
CAPACITY_NOISE, CAPACITY_EXTRA = 0.0, 2


def capacity_state():
    st = O.TronState(20, 2, 2)
    O.tron_reset(st, *O.tron_start_positions(20, 2))
    st.tcount[:] = [0, 2]                                        # (at noise 0 one coin of the avoid model tells the rows apart: 0 and 1 draw it alike)
    return st


# ---- the crash kinds of one tree step (tron_mcts_ref.CRASH_KINDS), each to be met by a player other than the seat on the
# way to a pending leaf under both models: (shape, noise) with B = 32, S = 30.  Three players give (a) to (c), four the
# head-on kinds, eight (on 49 and 81 cells) every kind including the head of a dead player
CRASH_CASES = [(7, 3), (5, 4), (7, 4), (7, 8), (9, 8)]
CRASH_B, CRASH_S = 32, 30


def crash_seats(P, B):
    """the players in turn on the even rows (the odd ones keep player 0, whose walk late_positions leaves free)"""
    s = (np.arange(B) // 2) % P
    s[np.arange(B) % 2 == 1] = 0
    return s.astype(np.int8)
