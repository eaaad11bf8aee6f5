"""Plain-Python restatement of crl_blokus_mcts ("batched tree search with progressive widening" in
include/colosseum_hip.h) over the CPU oracle's bindings: the plies are oracle.blokus_step's, the legal lists
oracle.blokus_valid's (tests/blokus_ref.py: blokus_one, blokus_list), the draws rng_ref.philox's.  Written from the
header's words, one position and one simulation at a time; no code is shared with the kernel.

`search` takes a one-game oracle state and returns (ids, visits, value, nodes, best) as Python lists / ints; `blokus_mcts`
runs it over a batch and returns numpy arrays shaped as the C outputs.  Neither writes its state."""
import math

import numpy as np

from oracle import oracle as O
from tests import rng_ref as RNG
from tests.blokus_ref import M32, _FIELDS, blokus_list, blokus_one

TAG = RNG.CRL_TAG_BLOKUS_PLAYOUT           # shared with crl_blokus_playout: the second counter word keeps them apart
PLAYOUT_BIT, WIDEN_BIT = 0x40000000, 0x80000000
NODE_BYTES, FIXED_BYTES, TREE_LDS = 24, 1280, 45056
S_MAX = min(65535, (TREE_LDS - FIXED_BYTES) // NODE_BYTES - 1)
MAX_DEPTH = 336


def cexp_of(exploration):
    return int(round(256.0 * float(exploration)))


def lg(n):
    """the contract's piecewise-linear log2 with 8 fraction bits, n >= 1"""
    m = n.bit_length() - 1
    return 256 * m + (((n << (31 - m)) & M32) >> 23 & 255)


def score(n_v, n_u, w_u, R, cexp):
    exploit = (w_u << 16) // (n_u * R)
    X = (lg(n_v) << 24) // n_u
    return exploit + ((cexp * math.isqrt(X)) >> 8)


def playout_word(seed, g, c, s, r):
    """the word of a leaf playout's ply at step counter c: simulation s, playout r"""
    return int(RNG.philox(g, (c >> 2) | PLAYOUT_BIT, (s << 16) | r, TAG, seed)[c & 3])


def widen_word(seed, g, d, s):
    """the word that draws a new child of a node at depth d in simulation s"""
    return int(RNG.philox(g, WIDEN_BIT | d, s, TAG, seed)[0])


def _copy(one):
    out = O.BlokusState(1)
    for name in _FIELDS:
        getattr(out, name)[0] = getattr(one, name)[0]
    return out


def _step(one, act):
    """one ply as crl_blokus_step plays it -> (terminal, winners mask)"""
    r, term, ws = O.blokus_step(one, np.array([act], np.int32))
    assert r[0] >= 0 or term[0], "an illegal ply"
    return bool(term[0]), int(ws[0])


def playout(one, seed, g, c, s, r):
    """crl_blokus_playout's random ply loop on `one` (mutated) under the search's counter words -> (winners mask, plies)"""
    plies = 0
    while True:
        ids = blokus_list(one)
        act = int(ids[(playout_word(seed, g, c, s, r) * len(ids)) >> 32]) if len(ids) else -1
        term, ws = _step(one, act)
        plies += 1
        c = (c + 1) & M32
        if term:
            return ws, plies


class Node:
    __slots__ = ("n", "w", "id", "rank", "term", "L", "slots")

    def __init__(self, id=-2, rank=0, term=False):
        self.n, self.w, self.id, self.rank, self.term, self.L, self.slots = 0, 0, id, rank, term, None, {}


def search(root, S, R, W=8, cexp=256, seed=0, g=0, tc=0, cand=None, count=None):
    """the tree of one position.  cand: a sequence of A dense ids, or None.  count: a dict whose 'plies' / 'playouts' grow
    by what the leaf playouts played, and which counts the edges the search went over: 'depth' the longest path in plies
    (a maximum), 'deep' the simulations whose path has 64 plies or more, 'sel_term' those that end on a terminal node
    reached by selection, 'probes' / 'wraps' the steps of the rank probe and those of them that go from L - 1 to 0, 'full'
    the expansions that give a node with L >= 1 legal actions its L-th child, 'deep_sel' the selections between two or more
    children below a node of depth 63 or more (they read n and w of nodes 64 plies or more down the path)."""
    assert 1 <= S <= S_MAX and 1 <= R <= 1024 and 1 <= W <= 64 and 0 <= cexp <= 65535

    def note(key, by=1):
        if count is not None:
            count[key] = count.get(key, 0) + by
    pl0 = int(root.to_move[0]) & 3
    K = W if cand is None else len(cand)
    top = Node()
    playable = []
    if cand is not None:
        assert 1 <= K <= 64
        legal, seen = set(int(i) for i in blokus_list(root)), set()
        for a, v in enumerate(cand):
            if int(v) in legal and int(v) not in seen:
                playable.append(a)
                seen.add(int(v))
        if not playable:
            return [-2] * K, [0] * K, [0] * K, 0, -2
    nodes = 1
    for s in range(S):
        one, v, d, path = _copy(root), top, 0, [top]
        while True:
            c = len(v.slots)
            if v is top and cand is not None:
                fresh = [a for a in playable if a not in v.slots]
                expand = bool(fresh)
            else:
                expand = c < W and c * c <= v.n and (c == 0 or c < max(v.L, 1))
            if expand:
                if v is top and cand is not None:
                    slot, act, rho = fresh[0], int(cand[fresh[0]]), 0
                else:
                    ids = blokus_list(one)
                    assert v.L is None or v.L == len(ids)
                    v.L, slot, act, rho = len(ids), c, -1, 0
                    if v.L:
                        rho = (widen_word(seed, g, d, s) * v.L) >> 32
                        taken = set(u.rank for u in v.slots.values())
                        while rho in taken:
                            note("probes")
                            note("wraps", int(rho + 1 == v.L))
                            rho = (rho + 1) % v.L
                        act = int(ids[rho])
                        note("full", int(c + 1 == v.L))
                term, ws = _step(one, act)
                u = Node(act, rho, term)
                v.slots[slot] = u
                nodes += 1
            else:
                slot = max(sorted(v.slots), key=lambda k: score(v.n, v.slots[k].n, v.slots[k].w, R, cexp))   # (the first of equals)
                u = v.slots[slot]
                note("deep_sel", int(d >= 63 and c >= 2))
                term, ws = _step(one, u.id)
                assert term == u.term
            d += 1
            path.append(u)
            if expand or term or d >= MAX_DEPTH:
                break
            v = u
        if count is not None:
            count["depth"] = max(count.get("depth", 0), d)
            note("deep", int(d >= 64))
            note("sel_term", int(term and not expand))
        if term:
            wins = [R * ((ws >> q) & 1) for q in range(4)]
        else:
            wins = [0, 0, 0, 0]
            for r in range(R):
                ws, plies = playout(_copy(one), seed, g, (tc + d) & M32, s, r)
                for q in range(4):
                    wins[q] += (ws >> q) & 1
                if count is not None:
                    count["plies"] = count.get("plies", 0) + plies
                    count["playouts"] = count.get("playouts", 0) + 1
        for i, node in enumerate(path):
            node.n += 1
            if i:
                node.w += wins[(pl0 + i - 1) & 3]
    ids = [top.slots[k].id if k in top.slots else -2 for k in range(K)]
    visits = [top.slots[k].n if k in top.slots else 0 for k in range(K)]
    value = [top.slots[k].w if k in top.slots else 0 for k in range(K)]
    best_slot = max(sorted(top.slots), key=lambda k: (top.slots[k].n, top.slots[k].w))
    return ids, visits, value, nodes, top.slots[best_slot].id


def blokus_mcts(st, S, R, W=8, cexp=256, seed=0, first_env_id=0, tcount=None, cand=None, count=None):
    """crl_blokus_mcts on the oracle state `st` -> ids int32 [B, K], visits, value uint32 [B, K], nodes uint32 [B], best int32 [B]"""
    B = st.B
    K = W if cand is None else np.asarray(cand).shape[1]
    ids, visits, value = np.zeros((B, K), np.int32), np.zeros((B, K), np.uint32), np.zeros((B, K), np.uint32)
    nodes, best = np.zeros(B, np.uint32), np.zeros(B, np.int32)
    for b in range(B):
        tc = 0 if tcount is None else int(tcount[b])
        out = search(blokus_one(st, b), S, R, W, cexp, seed, (first_env_id + b) & M32, tc,
                     None if cand is None else [int(x) for x in np.asarray(cand)[b]], count)
        ids[b], visits[b], value[b], nodes[b], best[b] = out
    return ids, visits, value, nodes, best
