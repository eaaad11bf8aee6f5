"""Numpy restatements of the Voronoi-territory contract (include/colosseum_hip.h, crl_tron_territory) and of the
territory-greedy agent on top of it (crl_tron_sample_territory).

Two independent restatements of the areas, both batched over instances (an instance = one position with at most one forced
seat):
  (i)  ``areas_by_distance``: one full breadth-first search per player through ALL free cells, then the strict-minimum
       comparison of the definition;
  (ii) ``areas_by_levels``: the level-synchronous flood through unclaimed cells only (what the kernels do).
Test infrastructure: the stepping is the CPU oracle's; ``rng_ref.philox`` is the vectorised Philox4x32-10 the host tests
check against the oracle's.
"""
import numpy as np

from tests import rng_ref as RNG
from tests import tron_ref

TAG_TERRITORY = RNG.CRL_TAG_TRON_TERRITORY
FATAL_SCORE = -(1 << 30)
_DX = np.array([0, 1, 0, -1])
_DY = np.array([-1, 0, 1, 0])
_TURN = np.array([0, 1, 3])          # candidates 0 forward, 1 right, 2 left as direction offsets


def first_cells(N, board, heads, dirs, deaths, seat=None, forced=None):
    """Instances from positions: board int8 [I, N*N], heads / dirs / deaths [P, I]; seat / forced int [I] or None (nobody
    forced).  -> (free bool [I, N, N], first bool [I, P, N, N], fatal bool [I]): the first cells of every live player (only
    the forced action's for the seat), already restricted to free cells on the board; fatal: the seat's forced cell is off
    the board or occupied."""
    I = board.shape[0]
    P = heads.shape[0]
    free = (board.reshape(I, N, N) == 0)
    first = np.zeros((I, P, N, N), dtype=bool)
    fatal = np.zeros(I, dtype=bool)
    rows = np.arange(I)
    h = np.clip(heads.astype(np.int64), 0, N * N - 1)
    x, y = h % N, h // N
    d = dirs.astype(np.int64) & 3
    for p in range(P):
        live = deaths[p] == 0
        for a in range(3):
            use = live.copy()
            if seat is not None:
                use &= (np.asarray(seat) != p) | (np.asarray(forced) == a)
            dd = (d[p] + _TURN[a]) & 3
            nx, ny = x[p] + _DX[dd], y[p] + _DY[dd]
            on = (nx >= 0) & (nx < N) & (ny >= 0) & (ny < N)
            cx, cy = np.clip(nx, 0, N - 1), np.clip(ny, 0, N - 1)
            ok = use & on & free[rows, cy, cx]
            first[rows[ok], p, cy[ok], cx[ok]] = True
            if seat is not None:
                is_forced = live & (np.asarray(seat) == p) & (np.asarray(forced) == a)
                fatal |= is_forced & ~(on & free[rows, cy, cx])
    return free, first, fatal


def _grow(f):
    """4-neighbour dilation of bool [..., N, N] (without the cells themselves)"""
    g = np.zeros_like(f)
    g[..., 1:, :] |= f[..., :-1, :]
    g[..., :-1, :] |= f[..., 1:, :]
    g[..., :, 1:] |= f[..., :, :-1]
    g[..., :, :-1] |= f[..., :, 1:]
    return g


def areas_by_distance(free, first):
    """(i): d_p(c) by one BFS per player through all free cells; area = cells where d_p is finite and strictly smallest.
    -> int32 [I, P]"""
    I, P, N, _ = first.shape
    INF = np.iinfo(np.int32).max
    dist = np.full((I, P, N, N), INF, dtype=np.int32)
    front = first.copy()
    level = 1
    while front.any():
        dist[front] = level
        level += 1
        front = _grow(front) & free[:, None] & (dist == INF)
    area = np.zeros((I, P), dtype=np.int32)
    for p in range(P):
        others = np.delete(dist, p, axis=1)
        best_other = others.min(axis=1) if P > 1 else np.full((I, N, N), INF, dtype=np.int32)
        area[:, p] = ((dist[:, p] < INF) & (dist[:, p] < best_other)).sum(axis=(1, 2))
    return area


def areas_by_levels(free, first):
    """(ii): the level-synchronous flood through unclaimed cells.  -> (int32 [I, P], depth int32 [I]: levels that claimed a
    cell)"""
    I, P, N, _ = first.shape
    free = free.copy()
    new = first & free[:, None]
    area = np.zeros((I, P), dtype=np.int32)
    depth = np.zeros(I, dtype=np.int32)
    for _ in range(N * N + 1):
        count = new.sum(axis=1)
        contested = count >= 2
        area += (new & ~contested[:, None]).sum(axis=(2, 3)).astype(np.int32)
        claimed = count >= 1
        if not claimed.any():
            break
        depth += claimed.any(axis=(1, 2))
        free &= ~claimed
        new = _grow(new) & free[:, None]
    return area, depth


def territory(N, board, heads, dirs, deaths, seat=None, cand=None, method="levels"):
    """The call's outputs for positions board [B, N*N], heads / dirs / deaths [P, B]: (area int32 [B, A, P], info uint8
    [B, A]); cand int [B, A] or None (A = 1, nobody forced), seat int [B] or None (player 0)."""
    B, P = board.shape[0], heads.shape[0]
    if cand is None:
        free, first, _ = first_cells(N, board, heads, dirs, deaths)
        area = areas_by_levels(free, first)[0] if method == "levels" else areas_by_distance(free, first)
        return area.reshape(B, 1, P), np.ones((B, 1), dtype=np.uint8)
    cand = np.asarray(cand, dtype=np.int64)
    A = cand.shape[1]
    sp = np.zeros(B, dtype=np.int64) if seat is None else np.asarray(seat, dtype=np.int64)
    in_range = (sp >= 0) & (sp < P)
    seat_live = in_range & (deaths[np.clip(sp, 0, P - 1), np.arange(B)] == 0)
    area = np.zeros((B, A, P), dtype=np.int32)
    info = np.zeros((B, A), dtype=np.uint8)
    for a in range(A):
        ev = seat_live & (cand[:, a] >= 0) & (cand[:, a] <= 2)
        idx = np.nonzero(ev)[0]
        if idx.size == 0:
            continue
        free, first, fatal = first_cells(N, board[idx], heads[:, idx], dirs[:, idx], deaths[:, idx], sp[idx], cand[idx, a])
        got = areas_by_levels(free, first)[0] if method == "levels" else areas_by_distance(free, first)
        area[idx, a] = got
        info[idx, a] = 1 | (fatal.astype(np.uint8) << 1)
    return area, info


def scores(area, info, deaths, seat):
    """The agent's score of every row: area [B, A, P], info [B, A], deaths [P, B], seat int [B] -> int64 [B, A]"""
    B, A, P = area.shape
    rows = np.arange(B)
    own = area[rows, :, seat].astype(np.int64)                              # [B, A]
    other_live = (deaths.T == 0)
    other_live[rows, seat] = False
    rival = np.where(other_live[:, None, :], area, 0).max(axis=2)
    return np.where((info & 2) != 0, FATAL_SCORE, own - rival)


def greedy_action(N, board, heads, dirs, deaths, seat):
    """The noise-free rule for seat [B] (live seats): the best-scoring candidate, ties to the lowest index -> int64 [B]"""
    B = board.shape[0]
    cand = np.tile(np.arange(3), (B, 1))
    area, info = territory(N, board, heads, dirs, deaths, seat, cand)
    return np.argmax(scores(area, info, deaths, np.asarray(seat)), axis=1)


def decide(N, board, heads, dirs, deaths, g, c, seed, noise, players=None):
    """Actions int8 [P, B] (0, +1, -1) of the territory-greedy agent for `players` (default: all); rows of other players and
    dead players are 0.  g, c: the games' global ids and step counters [B]."""
    P, B = heads.shape
    act = np.zeros((P, B), dtype=np.int8)
    thr = RNG.threshold(noise)
    code = np.array([0, 1, -1], dtype=np.int8)
    for p in (range(P) if players is None else players):
        w = RNG.philox(np.asarray(g, np.uint64), np.asarray(c, np.uint64), p, TAG_TERRITORY, seed)
        noisy = w[0].astype(np.uint64) < np.uint64(thr)
        a = RNG.mulhi(w[1], 3)
        live = deaths[p] == 0
        idx = np.nonzero(live & ~noisy)[0]
        if idx.size:
            a[idx] = greedy_action(N, board[idx], heads[:, idx], dirs[:, idx], deaths[:, idx], np.full(idx.size, p))
        act[p] = np.where(live, code[a], 0)
    return act


# ------------------------------------------------------------------ seeded mid-game positions (shared by the host and GPU tests)
def start_layout(N, P):
    """(heads, dirs) of the start layout: the oracle's ring, or, where it has no room (4x4 with more than four players), the
    first P cells of one colour of the checkerboard, everybody heading right"""
    from oracle import oracle as O
    if N == 4 and P > 4:
        return np.array([0, 2, 5, 7, 8, 10, 13, 15][:P], dtype=np.int16), np.ones(P, dtype=np.int8)
    return O.tron_start_positions(N, P)


def positions(N, P, B, seed, avoid, start=None):
    """B mid-game positions: game b stepped 0..~N plies with the oracle under random or avoid play (players that die stay
    dead; a game is kept at its last position with at least one live player... or none), from `start` = (heads, dirs),
    by default start_layout(N, P)"""
    from oracle import oracle as O
    sh, sd = start_layout(N, P) if start is None else start
    st = O.TronState(N, P, B)
    O.tron_reset(st, sh, sd)
    rng = np.random.default_rng(seed)
    stop = rng.integers(0, 2 * N, size=B)
    for t in range(int(stop.max())):
        if avoid:
            act = tron_ref.decide(N, st.board, st.heads, st.dirs, st.deaths, np.arange(B), np.full(B, t), seed, 0.1)
        else:
            act = rng.integers(-1, 2, size=(P, B)).astype(np.int8)
        nxt = st.copy()
        O.tron_step(nxt, act)
        go = stop > t
        st.board[go], st.heads[:, go], st.dirs[:, go], st.deaths[:, go] = nxt.board[go], nxt.heads[:, go], nxt.dirs[:, go], nxt.deaths[:, go]
    return st


# ------------------------------------------------------------------ hand-made positions (shared by the host and GPU tests)
def _pos(N, P, cells, heads_xy, dirs, deaths=None):
    """one position: `cells` int8 [N, N] (0 free; heads are stamped p + 1 on top), heads as (x, y)"""
    board = np.array(cells, dtype=np.int8).reshape(N, N).copy()
    heads = np.zeros((P, 1), dtype=np.int16)
    for p, (x, y) in enumerate(heads_xy):
        board[y, x] = p + 1
        heads[p, 0] = y * N + x
    k = np.zeros((P, 1), dtype=np.int8) if deaths is None else np.array(deaths, dtype=np.int8).reshape(P, 1)
    return {"N": N, "P": P, "board": board.reshape(1, N * N), "heads": heads,
            "dirs": np.array(dirs, dtype=np.int8).reshape(P, 1), "deaths": k}


def spiral_path(N):
    """the cells (x, y) of a one-cell-wide clockwise spiral corridor from the top-left corner inwards"""
    carved = np.zeros((N, N), dtype=bool)
    x, y, d = 0, 0, 1
    path = [(0, 0)]
    carved[0, 0] = True

    def can(x, y, d):
        nx, ny = x + _DX[d], y + _DY[d]
        if not (0 <= nx < N and 0 <= ny < N) or carved[ny, nx]:
            return False
        for e in range(4):                       # the new cell may touch the corridor only at the cell it comes from
            mx, my = nx + _DX[e], ny + _DY[e]
            if (mx, my) != (x, y) and 0 <= mx < N and 0 <= my < N and carved[my, mx]:
                return False
        return True

    while True:
        if not can(x, y, d):
            d = (d + 1) & 3
            if not can(x, y, d):
                return path
        x, y = x + _DX[d], y + _DY[d]
        carved[y, x] = True
        path.append((x, y))


def hand_boards():
    """name -> position dict (see the tests for the expected numbers)"""
    out = {}
    # a 3x3 pocket: ahead, right and left of the head are occupied, the cell BEHIND it and its row are free
    out["behind"] = _pos(3, 1, [[1, 1, 1], [1, 0, 1], [0, 0, 0]], [(1, 1)], [0])
    # player 0 walled in on all four sides, player 1 with the rest of a 5x5 board
    cells = np.zeros((5, 5), np.int8)
    cells[0, 1] = cells[1, 0] = cells[1, 2] = cells[2, 1] = 1
    out["walled"] = _pos(5, 2, cells, [(1, 1), (3, 3)], [0, 0])
    # a one-cell-wide spiral on 19x19, the player at its outer end
    path = spiral_path(19)
    cells = np.ones((19, 19), np.int8)
    for (x, y) in path:
        cells[y, x] = 0
    out["spiral"] = _pos(19, 1, cells, [path[0]], [1])
    # a corridor along row 3 of a 7x7 board met from both ends, with a side branch off its middle cell
    cells = np.full((7, 7), 3, np.int8)
    cells[3, :] = 0
    cells[2, 3] = cells[1, 3] = 0
    out["corridor"] = _pos(7, 2, cells, [(0, 3), (6, 3)], [1, 3])
    return out
