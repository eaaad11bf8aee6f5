"""Plain-Python restatement of crl_tron_puct_* (include/colosseum_hip.h, "tree search valued by the caller's network (PUCT),
Tron"), written from the header's words: a tree is plain lists, the integers are Python ints, isqrt is math.isqrt, "expanded"
is a flag of its own.  No code is shared with the kernels.  The positions, the tree step and the CLOSED rule are those of
tests/tron_mcts_ref.py (which tests/test_tron_mcts_host.py holds to oracle.tron_step); the observation of a leaf is
oracle.tron_observe on the leaf state.

A node's position is a pure function of the root and the edge sequence (the header says so), so the tree keeps every node's
position from the descent that made the node instead of replaying the edges in every descent; tests/test_tron_puct_host.py
replays them with oracle.tron_step.

`count`: a dict (see `new_count`) of what a search went over -- the deepest path, terminal leaves, nodes made on the way down,
backups with zero-sum priors, prior slots that hit the 65535 clamp, selects refused at capacity, and, under "crash_a" ..
"crash_g", the pending leaves on whose way from the root a player other than the seat met that crash kind of
tron_mcts_ref.CRASH_KINDS (so that its killer id is in the leaf that goes out) -- so that a test can require that its cases
reach the edges they name.

`evaluator`: the deterministic integer test evaluator, a pure function of (obs_board, obs_heads, obs_dirs) written once in
numpy, so that the host tests and the GPU tests apply the same function between select and backup."""
import math

import numpy as np

from oracle import oracle as O
from tests.rng_ref import M32, threshold
from tests.tron_mcts_ref import CRASH_KINDS, is_closed, pos_of, tree_step

FULL_VALUE, MAX_S = 65536, 4095


def new_count():
    count = {"depth": 0, "terminal": 0, "created": 0, "zero_sum": 0, "clamped": 0, "refused": 0}
    count.update(("crash_" + kind, 0) for kind in CRASH_KINDS)
    return count


def tree_bytes_floor(S_cap, N):
    """what any layout needs at least: the root board, and n, w, three prior slots and three child slots for S_cap + 1 nodes"""
    return N * N + (S_cap + 1) * 20


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

    def __init__(self, N, root, seat, tc, g, seed, agent, noise):
        P = len(root.h)
        self.N, self.P, self.seat, self.tc, self.g, self.agent = N, P, int(seat), int(tc) & M32, int(g) & M32, agent
        self.k0, self.k1, self.thr = seed & M32, (seed >> 32) & M32, threshold(noise)
        self.skipped = not 0 <= self.seat < P or root.k[self.seat] != 0 or (P >= 2 and root.n_alive() < 2)
        self.n, self.w = [0], [0]
        self.prior, self.child, self.expanded, self.where = [[0] * 3], [[0] * 3], [False], [root.copy()]
        self.sims = 0
        self.path, self.kind = None, None                        # kind: "pending" | "terminal"
        self.met = [frozenset()]                                 # per node: the crash kinds players other than the seat met on the way

    @property
    def nodes(self):
        return 0 if self.skipped else len(self.n)

    def select(self, S_cap, cpuct, fpu, count=None):
        """one descent; returns the pending leaf (position, depth) or None"""
        self.path, self.kind = None, None
        if self.skipped:
            return None
        if self.sims >= S_cap:
            if count is not None:
                count["refused"] += 1
            return None
        v, path = 0, [0]
        while True:
            if not self.expanded[v]:
                self.kind = "pending"
                break

            def key(e):
                u = self.child[v][e]
                return (score(self.n[v], self.n[u] if u else 0, self.w[u] if u else 0, self.prior[v][e], cpuct, fpu), -e)
            e = max(range(3), key=key)
            if not self.child[v][e]:
                pos = self.where[v].copy()
                step_count = {"events": []}
                tree_step(self.N, pos, self.seat, e, self.agent, self.thr, self.k0, self.k1, self.g,
                          (self.tc + len(path) - 1) & M32, step_count)
                self.met.append(self.met[v] | {kind for kind, who in step_count["events"] if who != self.seat})
                self.n.append(0), self.w.append(0), self.expanded.append(False)
                self.prior.append([0] * 3), self.child.append([0] * 3), self.where.append(pos)
                self.child[v][e] = len(self.n) - 1
                assert len(self.n) <= S_cap + 1
                if count is not None:
                    count["created"] += 1
            u = self.child[v][e]
            path.append(u)
            if is_closed(self.where[u], self.seat):
                self.kind = "terminal"
                if count is not None:
                    count["terminal"] += 1
                break
            v = u
        assert len(path) <= S_cap + 1
        self.path = path
        if count is not None:
            count["depth"] = max(count["depth"], len(path) - 1)
            if self.kind == "pending":
                for kind in self.met[path[-1]]:
                    count["crash_" + kind] += 1
        return (self.where[path[-1]], len(path) - 1) if self.kind == "pending" else None

    def edges(self):
        """the actions along the outstanding path"""
        return [self.child[a].index(b) for a, b in zip(self.path, self.path[1:])]

    def backup(self, prior, value, count=None):
        """prior: 3 ints (uint16), value: an int (int32), both read for a pending leaf only"""
        if self.skipped or self.path is None:
            return
        L = self.path[-1]
        if self.kind == "pending":
            total = sum(int(p) for p in prior)
            slots = []
            for a in range(3):
                raw = (int(prior[a]) << 16) // total if total else 65536 // 3
                if raw > 65535 and count is not None:
                    count["clamped"] += 1
                slots.append(min(65535, raw))
            if not total and count is not None:
                count["zero_sum"] += 1
            self.prior[L], self.expanded[L] = slots, True
            val = min(FULL_VALUE, max(0, int(value)))
        else:
            val = FULL_VALUE if self.where[L].k[self.seat] == 0 else 0
        for i, node in enumerate(self.path):
            self.n[node] += 1
            if i:
                self.w[node] += val
        self.sims += 1
        self.path, self.kind = None, None

    def root(self):
        """visits, value, prior [3], nodes, sims, best"""
        if self.skipped:
            return [0] * 3, [0] * 3, [0] * 3, 0, 0, -1
        kids = self.child[0]
        visits = [self.n[u] if u else 0 for u in kids]
        value = [self.w[u] if u else 0 for u in kids]
        best = -1
        if max(visits) > 0:
            best = max(range(3), key=lambda a: (visits[a], value[a], -a))
        return visits, value, list(self.prior[0]), len(self.n), self.sims, best


class Search:
    """the five entries on a batch: an oracle TronState in (never written), numpy arrays in the contract's layouts out"""

    def __init__(self, st, S_cap, seed=0, first_env_id=0, seat=None, agent="random", noise=0.1, use_tcount=True, count=None):
        assert 1 <= S_cap <= MAX_S and agent in ("random", "avoid")
        self.N, self.P, self.B, self.S_cap, self.count = st.N, st.P, st.B, S_cap, count
        self.seat = np.zeros(st.B, np.int8) if seat is None else np.asarray(seat, np.int8)
        self.trees = [Tree(st.N, pos_of(st, b), int(self.seat[b]), int(st.tcount[b]) if use_tcount else 0, first_env_id + b, seed,
                           agent, noise) for b in range(st.B)]

    def select(self, cpuct=256, fpu=32768):
        assert 0 <= cpuct <= 65535 and 0 <= fpu <= 65536
        B = self.B
        leaf = O.TronState(self.N, self.P, B)
        pending, depth, who = np.zeros(B, np.uint8), np.zeros(B, np.uint32), np.zeros(B, np.int8)
        for b, t in enumerate(self.trees):
            got = t.select(self.S_cap, cpuct, fpu, self.count)
            if got is None:
                continue
            pos, d = got
            leaf.board[b], leaf.heads[:, b], leaf.dirs[:, b], leaf.deaths[:, b] = pos.board, pos.h, pos.d, pos.k
            pending[b], depth[b], who[b] = 1, d, t.seat
        ob, oh, od, ok = O.tron_observe(leaf, who)               # (rows without a pending leaf are zeros in, zeros out)
        return {"obs_board": ob, "obs_heads": oh, "obs_dirs": od, "obs_deaths": ok, "pending": pending, "depth": depth,
                "leaf_board": leaf.board, "leaf_heads": leaf.heads, "leaf_dirs": leaf.dirs, "leaf_deaths": leaf.deaths}

    def backup(self, prior, value):
        for b, t in enumerate(self.trees):
            t.backup(prior[b], value[b], self.count)

    def root(self):
        B = self.B
        out = {"visits": np.zeros((B, 3), np.uint32), "value": np.zeros((B, 3), np.uint32), "prior": np.zeros((B, 3), np.uint32),
               "nodes": np.zeros(B, np.uint32), "sims": np.zeros(B, np.uint32), "best": np.full(B, -1, np.int32)}
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


MODES = ("mix", "zero", "clamp", "wild", "uniform", "win")


def evaluator(obs_board, obs_heads, obs_dirs, mode="mix"):
    """(obs_board int8 [B, N*N], obs_heads int16 [P, B], obs_dirs int8 [P, B]) -> (prior uint16 [B, 3], value int32 [B]).
    mix: hashed priors and values in [0, 65536]; zero: all-zero priors; clamp: one action (hashed) with prior 65535, the
    others 0; wild: values from far outside [0, 65536]; uniform: the constant evaluator (equal priors, value 32768); win:
    equal priors, value 65536."""
    board, heads, dirs = np.asarray(obs_board), np.asarray(obs_heads), np.asarray(obs_dirs)
    B, cells = board.shape
    h = _mix(np.full(B, 7 * 0x9E3779B1, np.uint64))
    for p in range(heads.shape[0]):
        h = _mix(h * 31 + (heads[p].astype(np.int64) + 40000).astype(np.uint64) * 4 + (dirs[p].astype(np.int64) & 3).astype(np.uint64))
    # the board as a weighted sum (one pass: the boards go up to 67 x 67)
    wgt = (np.arange(1, cells + 1, dtype=np.uint64) * 0x85EBCA6B) & 0xFFFFFFFF
    h = _mix(h + ((board.astype(np.int64) + 2).astype(np.uint64) * wgt[None, :]).sum(axis=1))
    prior = np.stack([_mix(h + 0x27D4EB2F * (a + 1)) >> 16 for a in range(3)], axis=1)
    value = (_mix(h + 0x165667B1) % 65537).astype(np.int64)
    if mode == "zero":
        prior[:] = 0
    elif mode == "clamp":
        one = (h % 3).astype(np.int64)
        prior[:] = 0
        prior[np.arange(B), one] = 65535
    elif mode == "wild":
        value = (value - 32768) * 40000                           # about +-1.3e9: far outside on both sides, and inside
    elif mode == "uniform":
        prior[:] = 1
        value[:] = 32768
    elif mode == "win":
        prior[:] = 1
        value[:] = FULL_VALUE
    else:
        assert mode == "mix"
    return prior.astype(np.uint16), value.astype(np.int32)


def run(st, S, S_cap=None, cpuct=256, fpu=32768, mode="mix", count=None, record=False, extra=0, **begin):
    """begin, S + extra x (select, evaluator, backup), root on the restatement: (root dict, [select dicts] if record)"""
    sr = Search(st, S_cap or S, count=count, **begin)
    seen = []
    for _ in range(S + extra):
        leaves = sr.select(cpuct, fpu)
        if record:
            seen.append(leaves)
        sr.backup(*evaluator(leaves["obs_board"], leaves["obs_heads"], leaves["obs_dirs"], mode))
    return sr.root(), seen
