"""numpy restatement of crl_ttt_playout / crl_blokus_playout (include/colosseum_hip.h, "batched random playouts") over the
CPU oracle's own bindings: oracle.ttt_step / blokus_step / blokus_valid and philox4x32.  Written from the header's words,
one playout at a time; no code is shared with the kernels.

States are the oracle's TTTState / BlokusState and are never written; ``tcount`` (uint32 [B] or None = 0) is the counter
base.  Both functions return numpy arrays shaped as the C outputs: wins uint32 [B, A, P], played / len_sum uint32 [B, A]
(and score_sum int32 [B, A, 4] for Blokus)."""
import numpy as np

from oracle import oracle as O

TAG_TTT_PLAYOUT = 0x54500000
TAG_BLOKUS_PLAYOUT = 0x42500000
LIST_CAP = 8192
M32 = 0xFFFFFFFF


def _key(seed):
    return [seed & M32, (seed >> 32) & M32]


def _rows(B, cand, A):
    if cand is None:
        assert A == 1
    else:
        cand = np.asarray(cand, np.int64)
        assert cand.shape == (B, A)
    return cand


# ------------------------------------------------------------------ TicTacToe
def ttt_word(seed, g, c, a, r):
    """the Philox word of step counter c for row candidate a, playout r: block c >> 3, word (c >> 1) & 3"""
    return int(O.philox4x32([g & M32, (c >> 3) & M32, ((a << 16) | r) & M32, TAG_TTT_PLAYOUT], _key(seed))[(c >> 1) & 3])


def ttt_draw(seed, g, c, a, r, empty, n_cells):
    """the random agent's cell: crl_ttt_rollout's even / odd rule and mulhi32 under the playout counter and tag"""
    cells = [i for i in range(n_cells) if (empty >> i) & 1]
    n = len(cells)
    w = ttt_word(seed, g, c, a, r)
    if c & 1:
        w = (w * (n + 1)) & M32
    return cells[(w * n) >> 32]


def _ttt_copy(st, b):
    one = O.TTTState(st.dims, st.K, st.P, 1)
    one.occ[:, 0] = st.occ[:, b]
    one.winner[0], one.to_move[0] = st.winner[b], st.to_move[b]
    return one


def _ttt_empty(one):
    return ((1 << one.n_cells) - 1) & ~int(np.bitwise_or.reduce(one.occ[:, 0]))


def ttt_one_playout(st, b, seed, g, c0, first, a, r):
    """(winner or -1, plies) of playout r of row (b, a); `first` the candidate cell or None"""
    one = _ttt_copy(st, b)
    plies, c = 0, c0
    if first is not None:
        _, term, ws = O.ttt_step(one, np.array([first], np.int8))
        plies = 1
        if term[0]:
            return int(ws[0]), plies
    while True:
        act = ttt_draw(seed, g, c, a, r, _ttt_empty(one), one.n_cells)
        _, term, ws = O.ttt_step(one, np.array([act], np.int8))
        plies += 1
        c = (c + 1) & M32
        if term[0]:
            return int(ws[0]), plies


def ttt_playout(st, seed, R, cand=None, A=1, first_env_id=0, tcount=None, rows=None):
    """crl_ttt_playout on the oracle state `st`.  rows: optional iterable of (b, a) to compute (the others stay 0)."""
    B, P, n = st.B, st.P, st.n_cells
    cand = _rows(B, cand, A)
    wins = np.zeros((B, A, P), np.uint32)
    played = np.zeros((B, A), np.uint32)
    len_sum = np.zeros((B, A), np.uint32)
    todo = rows if rows is not None else [(b, a) for b in range(B) for a in range(A)]
    for b, a in todo:
        empty = ((1 << n) - 1) & ~int(np.bitwise_or.reduce(st.occ[:, b]))
        if int(st.winner[b]) >= 0 or empty == 0 or not 0 <= int(st.to_move[b]) < P:
            continue                                         # a position that is over skips every row
        first = None
        if cand is not None:
            v = int(cand[b, a])
            if not (0 <= v < n and (empty >> v) & 1):
                continue                                     # not an empty cell: the row is skipped
            first = v
        c0 = 0 if tcount is None else int(tcount[b])
        g = first_env_id + b
        for r in range(R):
            w, plies = ttt_one_playout(st, b, seed, g, c0, first, a, r)
            if w >= 0:
                wins[b, a, w] += 1
            len_sum[b, a] += plies
        played[b, a] = R
    return wins, played, len_sum


# ------------------------------------------------------------------ Blokus
def blokus_word(seed, g, c, a, r):
    return int(O.philox4x32([g & M32, (c >> 2) & M32, ((a << 16) | r) & M32, TAG_BLOKUS_PLAYOUT], _key(seed))[c & 3])


def _blk_copy(st, b):
    one = O.BlokusState(1)
    for name in ("occ", "inv", "score", "round", "to_move"):
        getattr(one, name)[0] = getattr(st, name)[b]
    return one


def blokus_legal(one):
    """the mover's legal dense ids in reference order"""
    count, ids = O.blokus_valid(one, cap=LIST_CAP)
    assert count[0] <= LIST_CAP
    return ids[0, :count[0]]


def blokus_one_playout(st, b, seed, g, c0, first, a, r):
    """(winners mask, plies, final scores) of playout r of row (b, a); `first` the candidate id or None"""
    one = _blk_copy(st, b)
    plies, c = 0, c0
    if first is not None:
        _, term, ws = O.blokus_step(one, np.array([first], np.int32))
        plies = 1
        if term[0]:
            return int(ws[0]), plies, one.score[0].copy()
    while True:
        ids = blokus_legal(one)
        act = int(ids[(blokus_word(seed, g, c, a, r) * len(ids)) >> 32]) if len(ids) else -1
        _, term, ws = O.blokus_step(one, np.array([act], np.int32))
        plies += 1
        c = (c + 1) & M32
        if term[0]:
            return int(ws[0]), plies, one.score[0].copy()


def blokus_playout(st, seed, R, cand=None, A=1, first_env_id=0, tcount=None):
    """crl_blokus_playout on the oracle state `st`."""
    B = st.B
    cand = _rows(B, cand, A)
    wins = np.zeros((B, A, 4), np.uint32)
    played = np.zeros((B, A), np.uint32)
    len_sum = np.zeros((B, A), np.uint32)
    score_sum = np.zeros((B, A, 4), np.int32)
    for b in range(B):
        legal = set(int(i) for i in blokus_legal(_blk_copy(st, b))) if cand is not None else None
        c0 = 0 if tcount is None else int(tcount[b])
        for a in range(A):
            first = None
            if cand is not None:
                v = int(cand[b, a])
                if v not in legal:
                    continue                                 # not a legal dense id of the mover: the row is skipped
                first = v
            for r in range(R):
                mask, plies, score = blokus_one_playout(st, b, seed, first_env_id + b, c0, first, a, r)
                for p in range(4):
                    wins[b, a, p] += (mask >> p) & 1
                len_sum[b, a] += plies
                score_sum[b, a] += score
            played[b, a] = R
    return wins, played, len_sum, score_sum


# ------------------------------------------------------------------ exact values (3x3, two players, uniform random play)
_LINES_3X3 = [0b000000111, 0b000111000, 0b111000000, 0b001001001, 0b010010010, 0b100100100, 0b100010001, 0b001010100]


def exact_3x3(x, o, mover, memo=None):
    """(P(player 0 wins), P(player 1 wins)) of a running 3x3 position (marks x of player 0, o of player 1) under uniform
    random play to the end, by recursion over the game tree."""
    memo = {} if memo is None else memo
    key = (x, o, mover)
    if key in memo:
        return memo[key]
    empty = [i for i in range(9) if not ((x | o) >> i) & 1]
    p0 = p1 = 0.0
    for cell in empty:
        nx, no = (x | (1 << cell), o) if mover == 0 else (x, o | (1 << cell))
        mine = nx if mover == 0 else no
        if any((mine & ln) == ln for ln in _LINES_3X3):
            w = (1.0, 0.0) if mover == 0 else (0.0, 1.0)
        elif (nx | no) == 0x1FF:
            w = (0.0, 0.0)
        else:
            w = exact_3x3(nx, no, 1 - mover, memo)
        p0 += w[0] / len(empty)
        p1 += w[1] / len(empty)
    memo[key] = (p0, p1)
    return memo[key]


def reachable_3x3():
    """every running (non-terminal) position reachable from the empty 3x3 board: [(x, o, mover)] (4,520)"""
    seen, frontier = set(), [(0, 0, 0)]
    while frontier:
        nxt = []
        for x, o, m in frontier:
            if (x, o, m) in seen:
                continue
            seen.add((x, o, m))
            for cell in range(9):
                if ((x | o) >> cell) & 1:
                    continue
                nx, no = (x | (1 << cell), o) if m == 0 else (x, o | (1 << cell))
                mine = nx if m == 0 else no
                if any((mine & ln) == ln for ln in _LINES_3X3) or (nx | no) == 0x1FF:
                    continue
                nxt.append((nx, no, 1 - m))
        frontier = nxt
    return sorted(seen)
