"""Plain-Python restatement of crl_ttt_puct_* (include/colosseum_hip.h, "tree search valued by the caller's network"), written
from the header's words: a tree is plain lists, the integers are Python ints, isqrt is math.isqrt, "expanded" is a flag of
its own.  No code is shared with the kernels.  Positions go through tests/mcts_ref.Game (which test_ttt_mcts_host.py holds to
the oracle's ttt_step).

`count`: a dict (see `new_count`) of what a search went over -- the deepest path, terminal leaves, nodes made on the way down,
backups with zero-sum priors, prior slots that hit the 65535 clamp, selects refused at capacity -- so that a test can
require that its cases reach the edges they name.

`evaluator`: the deterministic integer test evaluator, a pure function of (relative board bytes, mover) written once in numpy,
so that the host tests and the GPU tests apply the same function between select and backup."""
import math

import numpy as np

from tests.mcts_ref import Game

FULL_VALUE, DRAW_VALUE, MAX_S = 65536, 32768, 4095


def new_count():
    return {"depth": 0, "terminal": 0, "created": 0, "zero_sum": 0, "clamped": 0, "refused": 0}


def tree_bytes_floor(S_cap, cells):
    """what any layout needs at least: n, w, a prior slot and a child slot per cell for S_cap + 1 nodes"""
    return (S_cap + 1) * (8 + 4 * cells)


def cpuct_of(exploration):
    return int(round(256 * exploration))


def fpu_of(fpu):
    return int(round(65536 * fpu))


def score(n_v, n_u, w_u, p_e, cpuct, fpu):
    exploit = w_u // n_u if n_u else fpu
    explore = (cpuct * p_e * math.isqrt(n_v << 16)) // ((1 + n_u) << 16)
    return exploit + explore


class Tree:
    """one tree; `begin` of the header"""

    def __init__(self, game, occ, winner, tm):
        self.game = game
        full = 0
        for o in occ:
            full |= o
        self.skipped = winner >= 0 or full == game.full or not 0 <= tm < game.P
        self.occ, self.tm = [int(o) for o in occ], int(tm)
        self.n, self.w = [0], [0]
        self.prior, self.child, self.expanded = [[0] * game.n], [[0] * game.n], [False]
        self.sims = 0
        self.path, self.kind, self.leaf = None, None, None       # kind: "pending" | "terminal"; leaf: (occ, mover, winner)

    @property
    def nodes(self):
        return 0 if self.skipped else len(self.n)

    def select(self, S_cap, cpuct, fpu, count=None):
        """one descent; returns the pending leaf (occ list, mover) or None"""
        game = self.game
        self.path, self.kind, self.leaf = None, None, None
        if self.skipped:
            return None
        if self.sims >= S_cap:
            if count is not None:
                count["refused"] += 1
            return None
        occ, tm, v, path = list(self.occ), self.tm, 0, [0]
        while True:
            if not self.expanded[v]:
                self.kind, ws = "pending", -1
                break
            full = 0
            for o in occ:
                full |= o
            E = [c for c in range(game.n) if not (full >> c) & 1]

            def key(e):
                u = self.child[v][e]
                return (score(self.n[v], self.n[u] if u else 0, self.w[u] if u else 0, self.prior[v][e], cpuct, fpu), -e)
            e = max(E, key=key)
            if not self.child[v][e]:
                self.n.append(0), self.w.append(0), self.expanded.append(False)
                self.prior.append([0] * game.n), self.child.append([0] * game.n)
                self.child[v][e] = len(self.n) - 1
                assert len(self.n) <= S_cap + 1
                if count is not None:
                    count["created"] += 1
            u = self.child[v][e]
            term, ws = game.step(occ, tm, e)
            tm = (tm + 1) % game.P
            path.append(u)
            if term:
                self.kind = "terminal"
                if count is not None:
                    count["terminal"] += 1
                break
            v = u
        assert len(path) <= game.n + 1
        self.path, self.leaf = path, (occ, tm, ws)
        if count is not None:
            count["depth"] = max(count["depth"], len(path) - 1)
        return (occ, tm) if self.kind == "pending" else None

    def backup(self, prior, value, count=None):
        """prior: cells ints (uint16), value: P ints (int32), both read for a pending leaf only"""
        game = self.game
        if self.skipped or self.path is None:
            return
        occ, m, ws = self.leaf
        if self.kind == "pending":
            full = 0
            for o in occ:
                full |= o
            E = [c for c in range(game.n) if not (full >> c) & 1]
            total = sum(int(prior[e]) for e in E)
            L = self.path[-1]
            slots = [0] * game.n
            for e in E:
                raw = (int(prior[e]) << 16) // total if total else 65536 // len(E)
                if raw > 65535 and count is not None:
                    count["clamped"] += 1
                slots[e] = min(65535, raw)
            if not total and count is not None:
                count["zero_sum"] += 1
            self.prior[L], self.expanded[L] = slots, True
            val = [0] * game.P
            for j in range(game.P):
                val[(m + j) % game.P] = min(FULL_VALUE, max(0, int(value[j])))
        else:
            val = [DRAW_VALUE if ws < 0 else (FULL_VALUE if p == ws else 0) for p in range(game.P)]
        for i, node in enumerate(self.path):
            self.n[node] += 1
            if i:
                self.w[node] += val[(self.tm + i - 1) % game.P]
        self.sims += 1
        self.path, self.kind, self.leaf = None, None, None

    def root(self):
        """visits, value, prior [cells], nodes, sims, best"""
        cells = self.game.n
        if self.skipped:
            return [0] * cells, [0] * cells, [0] * cells, 0, 0, -1
        kids = self.child[0]
        visits = [self.n[u] if u else 0 for u in kids]
        value = [self.w[u] if u else 0 for u in kids]
        best = -1
        if max(visits) > 0:
            best = max(range(cells), key=lambda c: (visits[c], value[c], -c))
        return visits, value, list(self.prior[0]), len(self.n), self.sims, best


def relative_board(game, occ, m, rel_mod):
    """crl_ttt_board's row for player m: -1 empty, else (owner - m) mod rel_mod"""
    row = [-1] * game.n
    for p, o in enumerate(occ):
        for c in range(game.n):
            if (o >> c) & 1:
                row[c] = (p - m) % rel_mod
    return row


class Search:
    """the five entries on a batch: an oracle TTTState (or anything with dims, K, P, B, occ [P, B], winner, to_move) in,
    numpy arrays in the contract's layouts out"""

    def __init__(self, st, S_cap, count=None):
        assert 1 <= S_cap <= MAX_S
        self.game = Game(st.dims, st.K, st.P)
        self.B, self.P, self.cells, self.S_cap, self.count = st.B, st.P, self.game.n, S_cap, count
        self.trees = [Tree(self.game, [int(x) for x in st.occ[:, b]], int(st.winner[b]), int(st.to_move[b])) for b in range(st.B)]

    def select(self, cpuct=256, fpu=32768, rel_mod=None):
        assert 0 <= cpuct <= 65535 and 0 <= fpu <= 65536
        rel_mod = rel_mod or self.P
        B, P, cells = self.B, self.P, self.cells
        out = {"board": np.zeros((B, cells), np.int8), "valid": np.zeros(B, np.uint32), "mover": np.full(B, -1, np.int8),
               "pending": np.zeros(B, np.uint8), "leaf_occ": np.zeros((P, B), np.uint32)}
        for b, t in enumerate(self.trees):
            leaf = t.select(self.S_cap, cpuct, fpu, self.count)
            if leaf is None:
                continue
            occ, m = leaf
            full = 0
            for o in occ:
                full |= o
            out["board"][b] = relative_board(self.game, occ, m, rel_mod)
            out["valid"][b] = self.game.full & ~full
            out["mover"][b], out["pending"][b] = m, 1
            out["leaf_occ"][:, b] = occ
        return out

    def backup(self, prior, value):
        for b, t in enumerate(self.trees):
            t.backup(prior[b], value[b], self.count)

    def root(self):
        B, cells = self.B, self.cells
        out = {"visits": np.zeros((B, cells), np.uint32), "value": np.zeros((B, cells), np.uint32),
               "prior": np.zeros((B, cells), np.uint32), "nodes": np.zeros(B, np.uint32), "sims": np.zeros(B, np.uint32),
               "best": np.full(B, -1, np.int32)}
        for b, t in enumerate(self.trees):
            out["visits"][b], out["value"][b], out["prior"][b], out["nodes"][b], out["sims"][b], out["best"][b] = t.root()
        return out


# ---- the test evaluator
def _mix(h):
    """a 32-bit integer mix (xor-shift-multiply rounds) on uint64 arrays holding 32-bit values"""
    h = h & 0xFFFFFFFF
    h = ((h ^ (h >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x846CA68B) & 0xFFFFFFFF
    return h ^ (h >> 16)


MODES = ("mix", "zero", "occupied", "clamp", "wild", "uniform")


def evaluator(board, mover, P, mode="mix"):
    """(board int8 [B, cells] relative to the mover, mover int8 [B]) -> (prior uint16 [B, cells], value int32 [B, P]).
    mix: hashed priors and values in [0, 65536]; zero: all-zero priors; occupied: priors non-zero on occupied cells only;
    clamp: one empty cell (the last) with prior 65535, the other empty cells 0; wild: values from far outside [0, 65536];
    uniform: the constant evaluator (equal priors, every value 32768)."""
    board, mover = np.asarray(board), np.asarray(mover)
    B, cells = board.shape
    h = _mix((mover.astype(np.int64) + 7).astype(np.uint64) * 0x9E3779B1)
    for c in range(cells):
        h = _mix(h * 31 + (board[:, c].astype(np.int64) + 2).astype(np.uint64) + 0x85EBCA6B * (c + 1))
    prior = np.stack([_mix(h + 0x27D4EB2F * (c + 1)) >> 16 for c in range(cells)], axis=1)
    value = np.stack([_mix(h + 0x165667B1 * (j + 1)) % 65537 for j in range(P)], axis=1).astype(np.int64)
    empty = board < 0
    if mode == "zero":
        prior[:] = 0
    elif mode == "occupied":
        prior = np.where(empty, 0, prior | 1)
    elif mode == "clamp":
        last = cells - 1 - np.argmax(empty[:, ::-1], axis=1)
        prior[:] = 0
        prior[np.arange(B), last] = 65535
    elif mode == "wild":
        value = (value - 32768) * 40000                           # about +-1.3e9: far outside on both sides, and inside
    elif mode == "uniform":
        prior[:] = 1
        value[:] = DRAW_VALUE
    else:
        assert mode == "mix"
    return prior.astype(np.uint16), value.astype(np.int32)


def run(st, S, S_cap=None, cpuct=256, fpu=32768, rel_mod=None, mode="mix", count=None, record=False, extra=0):
    """begin, S + extra x (select, evaluator, backup), root on the restatement: (root dict, [select dicts] if record)"""
    sr = Search(st, S_cap or S, count)
    seen = []
    for _ in range(S + extra):
        leaves = sr.select(cpuct, fpu, rel_mod)
        if record:
            seen.append(leaves)
        sr.backup(*evaluator(leaves["board"], leaves["mover"], st.P, mode))
    return sr.root(), seen
