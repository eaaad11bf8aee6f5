"""Plain-Python restatement of crl_blokus_puct_* ("tree search valued by the caller's network (PUCT), Blokus" in
include/colosseum_hip.h) over the CPU oracle's bindings: the plies are oracle.blokus_step's, the legal lists
oracle.blokus_valid's, the observations oracle.blokus_observe's, the draws rng_ref.philox's, the score tests/puct_ref.py's.
Written from the header's words, one tree and one simulation at a time; no code is shared with the kernels.

`Search` holds one Tree per row of an oracle state; `select` returns numpy arrays shaped as the C outputs, `backup` takes the
evaluator's, `root` returns the root rows.  `evaluator` is the integer hash the tests value leaves with, for numpy arrays and
for torch tensors alike."""
import numpy as np

from oracle import oracle as O
from tests import rng_ref as RNG
from tests.blokus_mcts_ref import _copy, _step
from tests.blokus_ref import blokus_list, blokus_one
from tests.puct_ref import score

TAG = RNG.CRL_TAG_BLOKUS_PLAYOUT
SELECT_KEYS = ("board", "pieces", "score", "cand", "n_cand", "n_legal", "mover", "pending", "depth", "leaf_occ", "leaf_inv",
               "leaf_score", "leaf_round", "leaf_to_move")
ROOT_KEYS = ("ids", "visits", "value", "prior", "nodes", "sims", "best")


def ranks(L, W, seed, g, tc, v):
    """the ranks of node v's candidates among L >= 1 legal actions"""
    if L <= W:
        return list(range(L))
    out = []
    for k in range(W):
        lo, hi = k * L // W, (k + 1) * L // W
        u = int(RNG.philox(g, 0xC0000000 | v, 0x80000000 | ((tc & 0x07FFFFFF) << 4) | (k >> 2), TAG, seed)[k & 3])
        out.append(lo + ((u * (hi - lo)) >> 32))
    return out


class Node:
    __slots__ = ("n", "w", "ids", "prior", "child", "term")

    def __init__(self, term=False):
        self.n, self.w, self.ids, self.prior, self.child, self.term = 0, 0, [], None, {}, term


class Tree:
    def __init__(self, one, S_cap, W, seed, g, tc):
        self.root, self.S_cap, self.W, self.seed, self.g, self.tc = _copy(one), S_cap, W, seed, g, tc
        self.nodes, self.sims, self.path, self.leaf = [Node()], 0, None, None

    def select(self, cpuct, fpu):
        """-> None, or (position, K ids, L, depth) of the pending leaf"""
        self.path = None
        if self.sims >= self.S_cap:
            return None
        pos, v, path = _copy(self.root), 0, [0]
        while True:
            node = self.nodes[v]
            if node.prior is None:                               # unexpanded: the pending leaf
                legal = blokus_list(pos)
                node.ids = [int(legal[r]) for r in ranks(len(legal), self.W, self.seed, self.g, self.tc, v)] if len(legal) else [-1]
                self.path, self.leaf = path, ("pending", int(pos.to_move[0]) & 3)
                return pos, node.ids, len(legal), len(path) - 1
            best, k = max((score(node.n, self.nodes[node.child[k]].n if k in node.child else 0,
                                 self.nodes[node.child[k]].w if k in node.child else 0, node.prior[k], cpuct, fpu), -k)
                          for k in range(len(node.ids)))
            k = -k
            term, ws = _step(pos, node.ids[k])
            if k not in node.child:
                node.child[k] = len(self.nodes)
                self.nodes.append(Node(term))
            v = node.child[k]
            assert self.nodes[v].term == term
            path.append(v)
            if term:
                self.path, self.leaf = path, ("terminal", ws)
                return None

    def backup(self, prior, value):
        if self.path is None:
            return
        kind, x = self.leaf
        m0 = int(self.root.to_move[0]) & 3
        if kind == "pending":
            leaf = self.nodes[self.path[-1]]
            K = len(leaf.ids)
            pr = [int(p) & 0xFFFF for p in prior[:K]]
            total = sum(pr)
            leaf.prior = [min(65535, (p << 16) // total if total else 65536 // K) for p in pr]
            val = [min(max(int(value[(q - x) & 3]), 0), 65536) for q in range(4)]
        else:
            val = [65536 if (x >> q) & 1 else 0 for q in range(4)]
        for i, v in enumerate(self.path):
            self.nodes[v].n += 1
            if i > 0:
                self.nodes[v].w += val[(m0 + i - 1) & 3]
        self.sims += 1
        self.path = None

    def root_row(self):
        W, r = self.W, self.nodes[0]
        ids, visits, value, prior = [-2] * W, [0] * W, [0] * W, [0] * W
        best = (0, 0, 0, -2)
        if r.prior is not None:
            for k, a in enumerate(r.ids):
                u = self.nodes[r.child[k]] if k in r.child else Node()
                ids[k], visits[k], value[k], prior[k] = a, u.n, u.w, r.prior[k]
                if u.n:
                    best = max(best, (u.n, u.w, -k, a))
        return ids, visits, value, prior, len(self.nodes), self.sims, best[3]


class Search:
    """`begin` on every row of the oracle state `st`"""

    def __init__(self, st, S_cap, W, seed=0, first_env_id=0, tcount=None):
        self.B, self.W = st.B, W
        self.trees = [Tree(blokus_one(st, b), S_cap, W, seed, (first_env_id + b) & 0xFFFFFFFF,
                           int(tcount[b]) if tcount is not None else 0) for b in range(st.B)]

    def select(self, cpuct=320, fpu=32768):
        B, W = self.B, self.W
        o = {"board": np.zeros((B, 20, 20), np.int8), "pieces": np.zeros((B, 4, 21), np.uint8), "score": np.zeros((B, 4), np.int32),
             "cand": np.full((B, W), -2, np.int32), "n_cand": np.zeros(B, np.int32), "n_legal": np.zeros(B, np.int32),
             "mover": np.full(B, -1, np.int8), "pending": np.zeros(B, np.uint8), "depth": np.zeros(B, np.int32),
             "leaf_occ": np.zeros((B, 4, 20), np.uint32), "leaf_inv": np.zeros((B, 4), np.uint32),
             "leaf_score": np.zeros((B, 4), np.int32), "leaf_round": np.zeros(B, np.int32), "leaf_to_move": np.zeros(B, np.int32)}
        for b, t in enumerate(self.trees):
            leaf = t.select(cpuct, fpu)
            if leaf is None:
                continue
            pos, ids, L, depth = leaf
            m = int(pos.to_move[0]) & 3
            ob, op, osc = O.blokus_observe(pos, np.array([m], np.int8))
            o["board"][b], o["pieces"][b], o["score"][b] = ob[0], op[0], osc[0]
            o["cand"][b, :len(ids)] = ids
            o["n_cand"][b], o["n_legal"][b], o["mover"][b], o["pending"][b], o["depth"][b] = len(ids), L, m, 1, depth
            o["leaf_occ"][b], o["leaf_inv"][b], o["leaf_score"][b] = pos.occ[0], pos.inv[0], pos.score[0]
            o["leaf_round"][b], o["leaf_to_move"][b] = pos.round[0], pos.to_move[0]
        return o

    def backup(self, prior, value):
        for b, t in enumerate(self.trees):
            t.backup(prior[b], value[b])

    def root(self):
        rows = [t.root_row() for t in self.trees]
        return {k: np.array([r[i] for r in rows], np.int64) for i, k in enumerate(ROOT_KEYS)}


def evaluator(leaves):
    """an integer hash of the leaf's board, candidates and mover, in operations numpy arrays and torch tensors share:
    -> (prior int64 [B, W] in 0 .. 32748, value int64 [B, 4] in 0 .. 65536)"""
    board, cand, mover = leaves["board"], leaves["cand"], leaves["mover"]
    if isinstance(board, np.ndarray):
        i64 = lambda a: a.astype(np.int64)
        ar = lambda n: np.arange(n, dtype=np.int64)
    else:
        import torch
        i64 = lambda a: a.to(torch.int64)
        ar = lambda n: torch.arange(n, dtype=torch.int64, device=board.device)
    B, W = cand.shape
    h = ((i64(board).reshape(B, 400) + 2) * (ar(400) % 251 + 1)).sum(1) + (i64(mover) + 1) * 977
    prior = (h.reshape(B, 1) * 31 + (i64(cand) + 3) * 7919 + ar(W).reshape(1, W) * 13) % 32749
    value = (h.reshape(B, 1) * 131 + ar(4).reshape(1, 4) * 40503) % 65537
    return prior, value
