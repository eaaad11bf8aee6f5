"""Plain-Python restatement of crl_ttt_mcts (include/colosseum_hip.h, "batched Monte Carlo tree search"), written from the
header's words: a tree is plain lists, the integers are Python ints, isqrt is math.isqrt.  No code is shared with the kernel.

It sits over the CPU oracle: positions are the oracle's TTTState, the win lines are oracle.ttt_lines.  For speed (a search
is some thousand playouts) the plies are stepped with masks of its own (`Game.step`) and the draws come from the integer
Philox of tests/rng_ref.py; tests/test_ttt_mcts_host.py holds both to oracle.ttt_step on whole random games and to
oracle.philox4x32.
`ttt_mcts(..., stepper="oracle")` runs the same search through oracle.ttt_step and oracle.philox4x32 themselves."""
import math

import numpy as np

from oracle import oracle as O
from tests.rng_ref import CRL_TAG_TTT_MCTS as TAG_TTT_MCTS, M32, philox_int as philox


def max_simulations(cells):
    """S_max of the header"""
    return min(4095, 65536 // (8 + 2 * cells) - 1)


def cexp_of(exploration):
    """TTTBatch.mcts's exploration -> cexp"""
    return int(round(256 * exploration))


def lg(n):
    """the header's piecewise-linear log2 with 8 fraction bits, n >= 1"""
    m = n.bit_length() - 1
    return 256 * m + (((n << (31 - m)) >> 23) & 255)


def score(n_v, n_u, w_u, R, cexp):
    exploit = (w_u << 15) // (n_u * R)
    X = (lg(n_v) << 24) // n_u
    return exploit + ((cexp * math.isqrt(X)) >> 8)


def _philox_oracle(c0, c1, c2, c3, k0, k1):
    return tuple(int(x) for x in O.philox4x32([c0, c1, c2, c3], [k0, k1]))


class Game:
    """a board: cells, the full mask, and per cell the win lines through it (oracle.ttt_lines)"""

    def __init__(self, dims, K, P):
        self.dims, self.K, self.P = tuple(int(d) for d in dims), int(K), int(P)
        d = (1,) * (3 - len(self.dims)) + self.dims
        self.n = d[0] * d[1] * d[2]
        self.full = (1 << self.n) - 1
        lines = [int(m) for m in O.ttt_lines(d[0], d[1], d[2], self.K)]
        self.lines_at = [[m for m in lines if (m >> c) & 1] for c in range(self.n)]

    def step(self, occ, tm, cell):
        """the ply `cell` (an empty one) of player tm on a running game, occ a list of P masks, changed in place:
        (terminal, winner or -1), as crl_ttt_step reports them"""
        mine = occ[tm] | (1 << cell)
        occ[tm] = mine
        for m in self.lines_at[cell]:
            if mine & m == m:
                return True, tm
        full = 0
        for o in occ:
            full |= o
        return full == self.full, -1

    def step_oracle(self, occ, tm, cell):
        """the same ply through oracle.ttt_step"""
        st = O.TTTState(self.dims, self.K, self.P, 1)
        st.occ[:, 0], st.to_move[0] = occ, tm
        _, term, ws = O.ttt_step(st, np.array([cell], np.int8))
        occ[:] = [int(x) for x in st.occ[:, 0]]
        assert int(st.to_move[0]) == (tm + 1) % self.P
        return bool(term[0]), int(ws[0])


def _empty_cells(game, occ):
    full = 0
    for o in occ:
        full |= o
    return [c for c in range(game.n) if not (full >> c) & 1]


def playout(game, occ, tm, seed, g, c, c2, tag=TAG_TTT_MCTS, step=None, rng=philox, count=None):
    """one random playout from the running position (occ, tm) to its first terminal ply: the winner or -1.  The first ply
    has step counter c; the draws are crl_ttt_rollout's under the third counter word c2 and `tag`.  `count`: a dict whose
    'playouts' and 'plies' are added to."""
    step = step or game.step
    occ = list(occ)
    k0, k1 = seed & M32, (seed >> 32) & M32
    block, words = None, None
    plies = 0
    while True:
        plies += 1
        cells = _empty_cells(game, occ)
        n = len(cells)
        if block != c >> 3:
            block = c >> 3
            words = rng(g & M32, block, c2, tag, k0, k1)
        w = words[(c >> 1) & 3]                                  # the draw rule of ttt_ref.random_agent, on ints
        if c & 1:
            w = (w * (n + 1)) & M32
        term, ws = step(occ, tm, cells[(w * n) >> 32])
        if term:
            if count is not None:
                count["playouts"] += 1
                count["plies"] += plies
            return ws
        tm = (tm + 1) % game.P
        c = (c + 1) & M32


def search(game, occ0, tm0, S, R, cexp, seed, g, tc, stepper="fast", count=None):
    """one tree from the running position (occ0, tm0): (visits [cells], value [cells], nodes, best)"""
    step = game.step if stepper == "fast" else game.step_oracle
    rng = philox if stepper == "fast" else _philox_oracle
    P, cells = game.P, game.n
    n, w, child = [0], [0], [[None] * cells]
    for s in range(S):
        occ, tm, v = list(occ0), tm0, 0
        path = [0]
        while True:
            E = _empty_cells(game, occ)
            fresh = [e for e in E if child[v][e] is None]
            if fresh:                                            # expand
                e = fresh[0]
                n.append(0), w.append(0), child.append([None] * cells)
                u = child[v][e] = len(n) - 1
            else:                                                # select
                e = max(E, key=lambda cell: (score(n[v], n[child[v][cell]], w[child[v][cell]], R, cexp), -cell))
                u = child[v][e]
            term, ws = step(occ, tm, e)
            tm = (tm + 1) % P
            path.append(u)
            if fresh or term:
                break
            v = u
        d = len(path) - 1
        wins, draws = [0] * P, 0
        if term:
            if ws >= 0:
                wins[ws] = R
            else:
                draws = R
        else:
            for r in range(R):
                ws = playout(game, occ, tm, seed, g, (tc + d) & M32, (s << 16) | r, step=step, rng=rng, count=count)
                if ws >= 0:
                    wins[ws] += 1
                else:
                    draws += 1
        for i, node in enumerate(path):
            n[node] += 1
            if i:
                w[node] += 2 * wins[(tm0 + i - 1) % P] + draws
    visits = [n[u] if u is not None else 0 for u in child[0]]
    value = [w[u] if u is not None else 0 for u in child[0]]
    best = max(range(cells), key=lambda cell: (visits[cell], value[cell], -cell) if child[0][cell] is not None else (-1, 0, 0))
    return visits, value, len(n), best


def ttt_mcts(st, S, R, cexp=256, seed=0, first_env_id=0, tcount=None, stepper="fast", count=None):
    """crl_ttt_mcts on the oracle state `st` (never written): visits, value uint32 [B, cells], nodes uint32 [B], best int32 [B].
    `count`: a dict {'playouts', 'plies'} that the random playouts played are added to."""
    game = Game(st.dims, st.K, st.P)
    B, n = st.B, game.n
    assert 1 <= S <= max_simulations(n) and 1 <= R <= 1024 and 0 <= cexp <= 65535
    visits, value = np.zeros((B, n), np.uint32), np.zeros((B, n), np.uint32)
    nodes, best = np.zeros(B, np.uint32), np.full(B, -1, np.int32)
    for b in range(B):
        occ = [int(x) for x in st.occ[:, b]]
        full = 0
        for o in occ:
            full |= o
        tm = int(st.to_move[b])
        if int(st.winner[b]) >= 0 or full == game.full or not 0 <= tm < st.P:
            continue                                             # a skipped position: zeros, nodes 0, best -1
        tc = 0 if tcount is None else int(tcount[b])
        visits[b], value[b], nodes[b], best[b] = search(game, occ, tm, S, R, cexp, seed, first_env_id + b, tc, stepper, count)
    return visits, value, nodes, best


def positions(dims, K, P, B, rng, tcounts=(3, 8, 2 ** 32 - 3), plies=None, plant=True):
    """An oracle state of B seeded mid-game positions: random plies (0 .. cells - 2 of them, or `plies` in every game) from
    the empty board through oracle.ttt_step, stopped where a game ends; then (`plant`) a few finished ones planted (a full
    board, a recorded winner) and two movers out of range, when B leaves room for them.  tcount: random, with `tcounts` in
    front (odd, even, and one that wraps inside a playout)."""
    st = O.TTTState(dims, K, P, B)
    n = st.n_cells
    for b in range(B):
        one = O.TTTState(dims, K, P, 1)
        for _ in range(int(rng.integers(0, n - 1)) if plies is None else plies):
            empty = [c for c in range(n) if not (int(np.bitwise_or.reduce(one.occ[:, 0])) >> c) & 1]
            before = (one.occ.copy(), int(one.to_move[0]))
            _, term, _ = O.ttt_step(one, np.array([rng.choice(empty)], np.int8))
            if term[0]:                                          # keep the running position before the last ply
                one.occ[:], one.to_move[0] = before
                one.winner[0] = -1
                break
        st.occ[:, b], st.winner[b], st.to_move[b] = one.occ[:, 0], one.winner[0], one.to_move[0]
    if plant and B >= 8:
        st.winner[B - 2] = int(st.to_move[B - 2])               # over: a recorded winner
        st.to_move[B - 3] = P                                    # a mover out of range
        st.to_move[B - 5] = -1
        full = (1 << n) - 1                                      # over: no empty cell
        st.occ[:, B - 4] = 0
        st.occ[0, B - 4] = full
    tc = rng.integers(0, 2 ** 32, size=B, dtype=np.uint64).astype(np.uint32)
    tc[:min(B, len(tcounts))] = np.array(tcounts[:B], np.uint64).astype(np.uint32)
    st.tcount[:] = tc
    return st


def late_positions(dims, K, P, B, rng, most=4):
    """An oracle state of B running positions with 1 .. `most` empty cells: the players move in turn to random cells that
    complete no line (a game in which every cell would is started again), so that the boards fill up without a winner."""
    game = Game(dims, K, P)
    st = O.TTTState(dims, K, P, B)
    b = 0
    while b < B:
        occ, tm, left = [0] * P, 0, int(rng.integers(1, most + 1))
        while game.n - bin(sum(occ)).count("1") > left:
            quiet = [c for c in _empty_cells(game, occ) if not game.step(list(occ), tm, c)[0]]
            if not quiet:
                break
            game.step(occ, tm, int(rng.choice(quiet)))
            tm = (tm + 1) % P
        else:
            st.occ[:, b], st.to_move[b] = occ, tm
            b += 1
    st.tcount[:] = rng.integers(0, 2 ** 32, size=B, dtype=np.uint64).astype(np.uint32)
    return st
