"""Plain-Python restatement of crl_tron_mcts (include/colosseum_hip.h, "batched tree search for a seat"), written from the
header's words: a tree is plain lists, the integers are Python ints, isqrt is math.isqrt.  No code is shared with the kernel.

A search is some thousand playouts of some dozen steps, so the steps and the two agents are restated here on Python ints
(`step`, `model_actions`, over the integer Philox of tests/rng_ref.py); tests/test_tron_mcts_host.py holds them to
oracle.tron_step, to tron_ref.decide / tron_ref.random_actions and to tron_ref.tron_playout.  A node's position is a pure
function of the root and the edge sequence (the header says so), so the tree keeps every node's position from the simulation
that made the node instead of replaying the edges in every descent."""
import math

import numpy as np

from tests.rng_ref import CRL_TAG_TRON_AVOID_PLAYOUT, CRL_TAG_TRON_PLAYOUT, M32, philox_int, threshold

TREE_STEP = 0xFFFF0000                       # the third counter word of the tree steps
_POW3 = (1, 3, 9, 27, 81, 243, 729, 2187)
_DX, _DY = (0, 1, 0, -1), (-1, 0, 1, 0)      # 0 N(y-1) 1 E(x+1) 2 S(y+1) 3 W(x-1)
_ACT = (0, 1, -1)                            # 0 forward, 1 right, 2 left in crl_tron_step's encoding


def max_simulations(N):
    """S_max of the header (below 1: the board is not supported)"""
    nwords = (N * N + 31) // 32
    return min(4095, (65536 - 264 * nwords) // 16 - 1)


def wave_bytes(N, S):
    """LDS of one wave's search (header: 16 bytes per node, 66 bitboards)"""
    return 16 * (S + 1) + 264 * ((N * N + 31) // 32)


def waves_per_workgroup(N, S, B):
    """one to four waves, as many as fit in 64 KB (and no more than there are games)"""
    return min(4, 65536 // wave_bytes(N, S), B)


def cexp_of(exploration):
    """TronBatch.mcts's exploration -> cexp"""
    return int(round(256 * exploration))


def lg(n):
    """the header's piecewise-linear log2 with 8 fraction bits, n >= 1"""
    m = n.bit_length() - 1
    return 256 * m + (((n << (31 - m)) >> 23) & 255)


def score(n_v, n_u, w_u, R, cexp):
    exploit = (w_u << 15) // (n_u * R)
    X = (lg(n_v) << 24) // n_u
    return exploit + ((cexp * math.isqrt(X)) >> 8)


class Pos:
    """one position: board (list of N*N cell values), heads, dirs, deaths (lists of P ints)"""
    __slots__ = ("board", "h", "d", "k")

    def __init__(self, board, h, d, k):
        self.board, self.h, self.d, self.k = board, h, d, k

    def copy(self):
        return Pos(list(self.board), list(self.h), list(self.d), list(self.k))

    def n_alive(self):
        return sum(1 for x in self.k if x == 0)


def pos_of(st, b):
    """position b of an oracle TronState"""
    return Pos([int(x) for x in st.board[b]], [int(x) for x in st.heads[:, b]], [int(x) & 3 for x in st.dirs[:, b]],
               [int(x) for x in st.deaths[:, b]])


def step(N, pos, act, count=None):
    """crl_tron_step without reset, in place; act: P values of 0, +1, -1.  -> (terminal, winners mask).  `count`: a dict whose
    'head_on' (where it has one) grows by one for every move onto a head (the hit that also kills the owner of the head), and
    to whose list 'events' (where it has one) every crash of the step is added as (kind, player), the kinds being those of
    CRASH_KINDS"""
    P = len(pos.h)
    bd, h, d, k = pos.board, pos.h, pos.d, pos.k
    events = None if count is None else count.get("events")
    was_alive, moved = [x == 0 for x in k], [False] * P
    for i in range(P):
        if k[i] > 0:
            if events is not None and was_alive[i]:
                events.append(("g", i))                          # killed head-on by an earlier mover: no move, no turn
            continue
        x, y = h[i] % N, h[i] // N
        dr = (d[i] + act[i] + 4) % 4
        x, y = x + _DX[dr], y + _DY[dr]
        d[i] = dr
        if x < 0 or x >= N or y < 0 or y >= N:
            k[i] = i + 1
            if events is not None:
                events.append(("a", i))
        elif bd[y * N + x] > 0:
            enemy = bd[y * N + x]
            k[i] = enemy
            if h[enemy - 1] == y * N + x:
                if events is not None:                           # the owner of the head gets the mover's id: (d) alive, (e) dead
                    events.append(("d" if k[enemy - 1] == 0 else "e", enemy - 1))
                    if k[enemy - 1] == 0 and moved[enemy - 1]:
                        events.append(("f", i))                  # both went for the same free cell; the later one is i
                k[enemy - 1] = i + 1
                if count is not None and "head_on" in count:
                    count["head_on"] += 1
            elif events is not None:
                events.append(("c" if enemy == i + 1 else "b", i))
        else:
            bd[y * N + x] = i + 1
            h[i] = y * N + x
            moved[i] = True
    mask = 0
    for i in range(P):
        if k[i] == 0:
            mask |= 1 << i
    term = bin(mask).count("1") <= 1
    return term, (mask if term else 0)


# what can happen to a player in one step, by the killer id it leaves: (a) off the board: its own id; (b) into another
# player's trail: that player's id; (c) into its own trail: its own id; (d) the owner of a live head that a mover runs
# into: the mover's id (the mover gets the owner's); (e) the same for the head of a player that was dead already: its id is
# overwritten; (f) the later of two movers to one free cell, head-on against the earlier one's new head; (g) a player
# killed head-on by an earlier mover of the same step, at its own turn: it neither moves nor turns
CRASH_KINDS = ("a", "b", "c", "d", "e", "f", "g")


def _clamped(N, h, dr):
    x, y = h % N, h // N
    return min(max(y + _DY[dr & 3], 0), N - 1) * N + min(max(x + _DX[dr & 3], 0), N - 1)


def model_actions(N, pos, agent, thr, k0, k1, g, c, c2):
    """the agent's action (0, +1, -1) for every player on the pre-step position at step counter c, third counter word c2;
    dead players get 0 (their draws are not used)"""
    P = len(pos.h)
    out = [0] * P
    if agent == "avoid":
        for p in range(P):
            if pos.k[p]:
                continue
            w = philox_int(g, c, c2, CRL_TAG_TRON_AVOID_PLAYOUT | p, k0, k1)
            if w[0] < thr:
                out[p] = _ACT[(w[1] * 3) >> 32]
                continue
            occ = lambda off: pos.board[_clamped(N, pos.h[p], pos.d[p] + off)] > 0
            if not occ(0):
                out[p] = 0
            elif w[2] >> 31:                                     # (-1, left, right)
                out[p] = -1 if not occ(3) else 1
            else:                                                # (+1, right, left)
                out[p] = 1 if not occ(1) else -1
    else:
        j = c & 7
        for q in range((P + 3) // 4):
            word = philox_int(g, c >> 3, c2, CRL_TAG_TRON_PLAYOUT | q, k0, k1)[j >> 1]
            for i in range(4):
                p = 4 * q + i
                if p < P and not pos.k[p]:
                    out[p] = _ACT[(((word * _POW3[(j & 1) * 4 + i]) & M32) * 3) >> 32]
    return out


def tree_step(N, pos, seat, e, agent, thr, k0, k1, g, c, count=None):
    """the tree step with edge action e at step counter c, in place: the seat plays e, the others the model agent"""
    act = model_actions(N, pos, agent, thr, k0, k1, g, c, TREE_STEP)
    act[seat] = _ACT[e]
    return step(N, pos, act, count)


def is_closed(pos, seat):
    return pos.k[seat] != 0 or pos.n_alive() <= 1


def playout(N, pos, seat, agent, thr, k0, k1, g, c, c2, max_steps, count=None):
    """one playout from `pos` as it stands (never written): the seat's half-points.  The first step has counter c."""
    pos = pos.copy()
    length = 0
    while True:
        term, wm = step(N, pos, model_actions(N, pos, agent, thr, k0, k1, g, c, c2), count)
        length += 1
        if term or pos.k[seat] or (max_steps and length == max_steps):
            if count is not None:
                count["playouts"] += 1
                count["steps"] += length
            if term:
                return 2 if (wm >> seat) & 1 else 0
            return 0 if pos.k[seat] else 1
        c = (c + 1) & M32


def search(N, root, seat, S, R, cexp, agent, noise, max_steps, seed, g, tc, count=None):
    """one tree from `root` (never written): (visits [3], value [3], nodes, best).  `count`: a dict whose 'playouts', 'steps',
    'depth' (summed leaf depths), 'closed' (closed leaves) and 'head_on' (moves onto a head, in tree steps and playouts) are
    added to."""
    k0, k1, thr = seed & M32, (seed >> 32) & M32, threshold(noise)
    n, w, child, where, closed = [0], [0], [[None] * 3], [root], [False]
    for s in range(S):
        v, path = 0, [0]
        while True:
            fresh = [a for a in range(3) if child[v][a] is None]
            if fresh:                                            # expand
                e = fresh[0]
                pos = where[v].copy()
                tree_step(N, pos, seat, e, agent, thr, k0, k1, g, (tc + len(path) - 1) & M32, count)
                n.append(0), w.append(0), child.append([None] * 3), where.append(pos), closed.append(is_closed(pos, seat))
                u = child[v][e] = len(n) - 1
            else:                                                # select
                e = max(range(3), key=lambda a: (score(n[v], n[child[v][a]], w[child[v][a]], R, cexp), -a))
                u = child[v][e]
            path.append(u)
            if fresh or closed[u]:
                break
            v = u
        d, leaf = len(path) - 1, where[path[-1]]
        if closed[path[-1]]:
            total = R * (2 if leaf.k[seat] == 0 else 0)
        else:
            total = sum(playout(N, leaf, seat, agent, thr, k0, k1, g, (tc + d) & M32, (s << 16) | r, max_steps, count)
                        for r in range(R))
        if count is not None:
            count["depth"] += d
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
    return {"playouts": 0, "steps": 0, "depth": 0, "closed": 0, "head_on": 0}


def tron_mcts(st, S, R, cexp=256, seed=0, first_env_id=0, tcount=None, seat=None, agent="random", noise=0.1, max_steps=0,
              count=None):
    """crl_tron_mcts on the oracle state `st` (never written): visits, value uint32 [B, 3], nodes uint32 [B], best int32 [B]"""
    N, P, B = st.N, st.P, st.B
    assert 1 <= S <= max_simulations(N) and 1 <= R <= 1024 and 0 <= cexp <= 65535 and 0 <= max_steps <= 65535
    assert agent in ("random", "avoid")
    visits, value = np.zeros((B, 3), np.uint32), np.zeros((B, 3), np.uint32)
    nodes, best = np.zeros(B, np.uint32), np.full(B, -1, np.int32)
    for b in range(B):
        sp = 0 if seat is None else int(seat[b])
        root = pos_of(st, b)
        if not 0 <= sp < P or root.k[sp] != 0 or (P >= 2 and root.n_alive() < 2):
            continue                                             # a skipped position: zeros, nodes 0, best -1
        tc = 0 if tcount is None else int(tcount[b])
        visits[b], value[b], nodes[b], best[b] = search(N, root, sp, S, R, cexp, agent, noise, max_steps, seed,
                                                        (first_env_id + b) & M32, tc, count)
    return visits, value, nodes, best


# ---- positions for the tests
def positions(N, P, B, rng, most=None, noise=0.1, seed=5, tcounts=(3, 7, 8, 2 ** 32 - 3)):
    """An oracle TronState of B positions taken from avoid-agent games (tron_ref.HostLoop: the oracle's steps with
    auto-reset) after 0 .. `most` steps each (default N*N / P: from the start layout to nearly full boards), so that the
    fill levels differ and some seats are boxed in.  tcount: random, with `tcounts` in front."""
    from oracle import oracle as O
    from tests import tron_ref as TR
    sh, sd = O.tron_start_positions(N, P)
    loop = TR.HostLoop(N, P, B, sh, sd)
    most = max(1, (N * N) // max(P, 1) if most is None else most)
    target = rng.integers(0, most + 1, size=B)
    out = O.TronState(N, P, B)
    for t in range(int(target.max()) + 1):
        take = target == t
        out.board[take], out.heads[:, take] = loop.st.board[take], loop.st.heads[:, take]
        out.dirs[:, take], out.deaths[:, take] = loop.st.dirs[:, take], loop.st.deaths[:, take]
        loop.step(seed, noise)
    tc = rng.integers(0, 2 ** 32, size=B, dtype=np.uint64).astype(np.uint32)
    tc[:min(B, len(tcounts))] = np.array(tcounts[:B], np.uint64).astype(np.uint32)
    out.tcount[:] = tc
    return out


def _free_path(N, board, head, length, rng):
    """up to `length` free cells in a self-avoiding walk from `head` (never through a cell of `board` that is taken)"""
    path, cur = [], head
    for _ in range(length):
        x, y = cur % N, cur // N
        nxt = [ny * N + nx for nx, ny in ((x, y - 1), (x + 1, y), (x, y + 1), (x - 1, y))
               if 0 <= nx < N and 0 <= ny < N and board[ny * N + nx] == 0 and ny * N + nx not in path]
        if not nxt:
            break
        cur = int(rng.choice(nxt))
        path.append(cur)
    return path


def late_positions(N, P, B, rng, most=3):
    """`positions` with the boards walled up: the seat (player 0) keeps a free walk of 1 .. `most` cells from its head, the
    last live other player one of three cells more, every other free cell is filled with trail.  The reachable tree is a
    few nodes, most of them closed."""
    st = positions(N, P, B, rng, most=max(1, N * N // (2 * max(P, 1))))
    for b in range(B):
        live = [p for p in range(P) if st.deaths[p, b] == 0]
        if 0 not in live:
            continue
        board = st.board[b]
        keep = _free_path(N, board, int(st.heads[0, b]), int(rng.integers(1, most + 1)), rng)
        others = [p for p in live if p != 0]
        if others:
            mark = board.copy()
            mark[keep] = 1
            keep = keep + _free_path(N, mark, int(st.heads[others[-1], b]), len(keep) + 3, rng)
        fill = board == 0
        fill[keep] = False
        board[fill] = (rng.integers(0, P, size=int(fill.sum())) + 1).astype(np.int8)
    return st
