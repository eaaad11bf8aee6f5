"""Plain-Python restatement of crl_tron_mcts_territory (include/colosseum_hip.h): crl_tron_mcts's tree with one Voronoi flood
of the leaf's position in the place of the playouts.  Built from the pieces of tests/tron_mcts_ref.py (positions, the tree
step, the CLOSED rule, the score) and of tests/territory_ref.py (first cells and the two area restatements); the descent loop
is this module's own.  Python ints and floor divisions only; no code is shared with the kernel.

The areas of a leaf come from one of three restatements, which tests/test_tron_mcts_territory_host.py holds to each other:
"levels" (territory_ref.areas_by_levels, the default), "distance" (territory_ref.areas_by_distance: one full search per
player, then the strict minimum), and "bits" (the level flood on Python ints, one bit per cell with a spare column per row:
some hundred times faster on 64x64, which is what lets the GPU tests check the largest trees)."""
import numpy as np

from tests import territory_ref as V
from tests.rng_ref import M32, threshold
from tests.tron_mcts_ref import is_closed, max_simulations, pos_of, score, tree_step

METHODS = ("levels", "distance", "bits")


def wave_bytes(N, S):
    """LDS of one wave's search: 16 bytes per node, the root and the working bitboard"""
    return 16 * (S + 1) + 8 * ((N * N + 31) // 32)


def _areas_numpy(N, pos, method):
    """(areas [P], levels that claimed a cell, is some reached cell contested) by territory_ref, occupancy = value > 0"""
    P = len(pos.h)
    occ = (np.array(pos.board, np.int64) > 0).astype(np.int8).reshape(1, N * N)
    col = lambda xs: np.array(xs, np.int64).reshape(P, 1)
    free, first, _ = V.first_cells(N, occ, col(pos.h), col(pos.d), col(pos.k))
    area, depth = V.areas_by_levels(free, first)
    if method == "distance":
        area = V.areas_by_distance(free, first)
    reached, _ = V.areas_by_levels(free, first.any(axis=1, keepdims=True))   # every player as one: the cells anybody reaches
    return [int(a) for a in area[0]], int(depth[0]), int(area[0].sum()) < int(reached[0, 0])


_DX, _DY = (0, 1, 0, -1), (-1, 0, 1, 0)


def _areas_bits(N, pos):
    """the same three by the level flood on Python ints: cell (x, y) is bit y (N + 1) + x, column N stays 0"""
    P, T = len(pos.h), N + 1
    rows = np.zeros((N, T), np.uint8)
    rows[:, :N] = ~(np.array(pos.board, np.int64).reshape(N, N) > 0)
    free = int.from_bytes(np.packbits(rows.reshape(-1), bitorder="little").tobytes(), "little")
    nw = [0] * P
    for p in range(P):
        if pos.k[p]:
            continue
        x, y = pos.h[p] % N, pos.h[p] // N
        for turn in (0, 1, 3):
            dr = (pos.d[p] + turn) & 3
            nx, ny = x + _DX[dr], y + _DY[dr]
            if 0 <= nx < N and 0 <= ny < N:
                nw[p] |= (1 << (ny * T + nx)) & free
    area, levels, contested = [0] * P, 0, False
    for _ in range(N * N + 1):
        once = twice = 0
        for f in nw:
            twice |= once & f
            once |= f
        if not once:
            break
        levels += 1
        contested |= twice != 0
        for p in range(P):
            area[p] += (nw[p] & ~twice).bit_count()
        free &= ~once
        nw = [((f << 1) | (f >> 1) | (f << T) | (f >> T)) & free for f in nw]
    return area, levels, contested


def leaf_areas(N, pos, method="levels"):
    assert method in METHODS
    return _areas_bits(N, pos) if method == "bits" else _areas_numpy(N, pos, method)


def leaf_value(N, pos, seat, Vs, method="levels", count=None):
    """the half-points of the OPEN leaf `pos` (never written) on the scale Vs"""
    area, levels, contested = leaf_areas(N, pos, method)
    a_s = area[seat]
    a_o = max([area[q] for q in range(len(area)) if q != seat and pos.k[q] == 0], default=0)
    if count is not None:
        count["flooded"] += 1
        count["levels"] += levels
        count["contested"] += bool(contested)
        count["empty"] += a_s + a_o == 0
    return Vs if a_s + a_o == 0 else (2 * Vs * a_s) // (a_s + a_o)


def search(N, root, seat, S, Vs, cexp, agent, noise, seed, g, tc, count=None, method="levels"):
    """one tree from `root` (never written): (visits [3], value [3], nodes, best)"""
    k0, k1, thr = seed & M32, (seed >> 32) & M32, threshold(noise)
    n, w, child, where, closed = [0], [0], [[None] * 3], [root], [False]
    for _ in range(S):
        v, path = 0, [0]
        while True:
            e = next((a for a in range(3) if child[v][a] is None), None)
            fresh = e is not None
            if fresh:                                            # expand: the lowest action without a child
                pos = where[v].copy()
                tree_step(N, pos, seat, e, agent, thr, k0, k1, g, (tc + len(path) - 1) & M32, count)
                n.append(0), w.append(0), child.append([None] * 3), where.append(pos), closed.append(is_closed(pos, seat))
                u = child[v][e] = len(n) - 1
            else:                                                # select: the best score, ties to the lowest action
                e = max(range(3), key=lambda a: (score(n[v], n[child[v][a]], w[child[v][a]], Vs, cexp), -a))
                u = child[v][e]
            path.append(u)
            if fresh or closed[u]:
                break
            v = u
        leaf = where[path[-1]]
        if closed[path[-1]]:
            total = 2 * Vs if leaf.k[seat] == 0 else 0
        else:
            total = leaf_value(N, leaf, seat, Vs, method, count)
        if count is not None:
            count["depth"] += len(path) - 1
            count["closed"] += bool(closed[path[-1]])
        for i, node in enumerate(path):
            n[node] += 1
            if i:
                w[node] += total
    visits = [n[u] if u is not None else 0 for u in child[0]]
    value = [w[u] if u is not None else 0 for u in child[0]]
    have = [a for a in range(3) if child[0][a] is not None]
    best = max(have, key=lambda a: (visits[a], value[a], -a)) if have else -1
    return visits, value, len(n), best


def new_count():
    """closed / flooded leaves, flooded leaves with a contested cell and with a_s + a_o == 0 ('empty'), summed leaf depths,
    summed flood levels, skipped positions, moves onto a head in the tree steps ('head_on')"""
    return {"closed": 0, "flooded": 0, "contested": 0, "empty": 0, "depth": 0, "levels": 0, "skipped": 0, "head_on": 0}


def tron_mcts_territory(st, S, Vs=256, cexp=256, seed=0, first_env_id=0, tcount=None, seat=None, agent="random", noise=0.1,
                        count=None, method="levels"):
    """crl_tron_mcts_territory on the oracle state `st` (never written): visits, value uint32 [B, 3], nodes uint32 [B], best
    int32 [B]"""
    N, P, B = st.N, st.P, st.B
    assert N <= 64 and 1 <= S <= max_simulations(N) and 1 <= Vs <= 1024 and 0 <= cexp <= 65535 and agent in ("random", "avoid")
    visits, value = np.zeros((B, 3), np.uint32), np.zeros((B, 3), np.uint32)
    nodes, best = np.zeros(B, np.uint32), np.full(B, -1, np.int32)
    for b in range(B):
        sp = 0 if seat is None else int(seat[b])
        root = pos_of(st, b)
        if not 0 <= sp < P or root.k[sp] != 0 or (P >= 2 and root.n_alive() < 2):
            if count is not None:
                count["skipped"] += 1
            continue                                             # a skipped position: zeros, nodes 0, best -1
        tc = 0 if tcount is None else int(tcount[b])
        visits[b], value[b], nodes[b], best[b] = search(N, root, sp, S, Vs, cexp, agent, noise, seed, (first_env_id + b) & M32,
                                                        tc, count, method)
    return visits, value, nodes, best


# ---- hand-made positions (shared by the host and the GPU tests); the expected numbers are worked out in the tests
def hand_state(N, P, heads_xy, dirs, free_xy):
    """an oracle TronState of one position: every cell is wall (value 1) but `free_xy`; heads as (x, y) carry p + 1"""
    from oracle import oracle as O
    st = O.TronState(N, P, 1)
    st.board[0, :] = 1
    for (x, y) in free_xy:
        st.board[0, y * N + x] = 0
    for p, (x, y) in enumerate(heads_xy):
        st.board[0, y * N + x] = p + 1
        st.heads[p, 0], st.dirs[p, 0] = y * N + x, dirs[p]
    return st


def corridor_state():
    """7x7, the seat at (1, 3) heading east: ahead a corridor of four cells, to its right one closed-in cell, to its left a
    corridor of three; the other player at (0, 6) heading east along the free bottom row"""
    free = [(x, 3) for x in (2, 3, 4, 5)] + [(1, 4)] + [(1, 2), (1, 1), (1, 0)] + [(x, 6) for x in range(1, 7)]
    return hand_state(7, 2, [(1, 3), (0, 6)], [1, 1], free)


def nowhere_state():
    """5x5, both players with one free cell ahead and walls everywhere else: after the step forward nobody has a first cell"""
    return hand_state(5, 2, [(1, 1), (1, 3)], [1, 1], [(2, 1), (2, 3)])


def head_on_state(P=2):
    """7x7.  Player 0 at (1, 3) heading east and player 1 at (3, 3) heading west, ONE free cell, (2, 3), between them; each
    has its own column free above and below it (x = 1 and x = 3, three cells each way), everything else is wall -- so (2, 3)
    is a dead end with walls above and below.  With P = 3 a bystander, player 2, stands at (5, 3) heading north with one
    free cell ahead, to its right and to its left."""
    free = [(2, 3)] + [(x, y) for x in (1, 3) for y in (0, 1, 2, 4, 5, 6)]
    if P == 2:
        return hand_state(7, 2, [(1, 3), (3, 3)], [1, 3], free)
    assert P == 3
    return hand_state(7, 3, [(1, 3), (3, 3), (5, 3)], [1, 3, 0], free + [(5, 2), (6, 3), (4, 3)])


def corner_state():
    """7x7, the seat in the corner (0, 0) heading north: forward and left leave the board, to its right the free top row
    (six cells); the other player at (0, 6) heading east with three free cells ahead of it along the bottom row"""
    return hand_state(7, 2, [(0, 0), (0, 6)], [0, 1], [(x, 0) for x in range(1, 7)] + [(x, 6) for x in (1, 2, 3)])


def pocket_state():
    """9x9, the seat at (4, 4) heading east.  Ahead: one cell, then a fork into two dead ends of five cells each (eleven
    cells to Voronoi, six of them can be played).  To its right (south): one winding corridor of nine cells.  To its left: a
    wall.  The other player at (0, 0) heads south down a corridor of seven cells."""
    fork = [(5, 4)] + [(6, 4), (7, 4), (8, 4), (8, 3), (8, 2)] + [(5, 3), (5, 2), (5, 1), (5, 0), (6, 0)]
    snake = [(4, 5), (4, 6), (4, 7), (4, 8), (5, 8), (6, 8), (7, 8), (8, 8), (8, 7)]
    return hand_state(9, 2, [(4, 4), (0, 0)], [1, 2], fork + snake + [(0, y) for y in range(1, 8)])
