"""Numpy restatement of crl_tron_playout's contract (include/colosseum_hip.h): R playouts per row (b, a) on private copies
of position b, the seat's forced first action, the random or avoid agent under the playout tags, the stop rules and the
four outputs.

Test infrastructure: the stepping is the CPU oracle's (``oracle.tron_step``, all copies at once; copies that have stopped
keep being stepped but are no longer counted); the agents' draws reuse ``avoid_ref.philox`` / ``clamped_cell``.
"""
import numpy as np

from tests import avoid_ref as AR

TAG_PLAYOUT = 0x54700000
TAG_AVOID_PLAYOUT = 0x54610000
_POW3 = np.array([1, 3, 9, 27, 81, 243, 729, 2187], np.uint64)
_M32 = np.uint64(0xFFFFFFFF)


def _mulhi3(w):
    return ((np.asarray(w, np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int64)


def random_actions(P, g, c, c2, seed):
    """int8 [P, M] of the random agent at counter c (uint32 [M]) for copies with game ids g and third words c2."""
    out = np.zeros((P, len(g)), np.int8)
    j = c & np.uint32(7)
    for q in range((P + 3) // 4):
        w = AR.philox(g, c >> np.uint32(3), c2, TAG_PLAYOUT | q, seed)
        word = np.choose((j >> np.uint32(1)).astype(np.int64), w).astype(np.uint64)
        for i in range(4):
            p = 4 * q + i
            if p >= P:
                break
            v = (word * _POW3[(j & np.uint32(1)).astype(np.int64) * 4 + i]) & _M32
            a3 = _mulhi3(v)
            out[p] = np.where(a3 == 2, -1, a3)
    return out


def avoid_actions(N, board, heads, dirs, deaths, g, c, c2, seed, noise):
    """int8 [P, M] of the avoid agent on the pre-step boards (as avoid_ref.decide, under the playout tag and counters)."""
    P, M = heads.shape
    thr = np.uint64(AR.threshold(noise))
    rows = np.arange(M)
    out = np.zeros((P, M), np.int8)
    occ = board > 0
    for p in range(P):
        w0, w1, w2, _ = AR.philox(g, c, c2, TAG_AVOID_PLAYOUT | p, seed)
        d = dirs[p].astype(np.int64)
        probe = lambda off: occ[rows, AR.clamped_cell(N, heads[p], d + off)]
        o_f, o_r, o_l = probe(0), probe(1), probe(3)
        a3 = _mulhi3(w1)
        noisy_act = np.where(a3 == 2, -1, a3)
        left_first = (w2 >> np.uint32(31)) != 0
        first_free = ~np.where(left_first, o_l, o_r)
        side = np.where(left_first == first_free, -1, 1)
        act = np.where(w0.astype(np.uint64) < thr, noisy_act, np.where(~o_f, 0, side))
        out[p] = np.where(deaths[p] != 0, 0, act)
    return out


def tron_playout(st, seed, R, cand=None, A=1, seat=None, tcount=None, first_env_id=0, agent="random", noise=0.1,
                 until="end", max_steps=0):
    """-> (wins [B, A, P], played [B, A], len_sum [B, A], ret_sum [B, A]) as int64, from the oracle state `st` (read only)."""
    from oracle import oracle as O
    N, P, B = st.N, st.P, st.B
    if cand is None:
        assert A == 1
        cand = np.full((B, 1), -1, np.int64)
        forced = False
    else:
        cand = np.asarray(cand, np.int64).reshape(B, A)
        forced = True
    seat = np.zeros(B, np.int64) if seat is None else np.asarray(seat, np.int64)
    tc = np.zeros(B, np.uint32) if tcount is None else np.asarray(tcount, np.uint32)
    # which rows play
    n_alive = (st.deaths == 0).sum(axis=0)
    ok_pos = (seat >= 0) & (seat < P)
    ok_pos &= np.array([st.deaths[s, b] == 0 if 0 <= s < P else False for b, s in enumerate(seat)])
    if P >= 2:
        ok_pos &= n_alive >= 2
    ok_row = ok_pos[:, None] & ((~forced) | ((cand >= 0) & (cand <= 2)))
    M = B * A * R
    bi = np.repeat(np.arange(B), A * R)
    ai = np.tile(np.repeat(np.arange(A), R), B)
    ri = np.tile(np.arange(R), B * A)
    cp = O.TronState(N, P, M)
    cp.board[:] = st.board[bi]
    cp.heads[:] = st.heads[:, bi]
    cp.dirs[:] = st.dirs[:, bi]
    cp.deaths[:] = st.deaths[:, bi]
    active = ok_row[bi, ai].copy()
    g = ((np.uint64(first_env_id) + bi.astype(np.uint64)) & _M32).astype(np.uint32)
    c2 = ((ai.astype(np.uint32) << np.uint32(16)) | ri.astype(np.uint32)).astype(np.uint32)
    ms = seat[bi].clip(0, P - 1)
    length = np.zeros(M, np.int64)
    ret = np.zeros(M, np.int64)
    won = np.zeros((M, P), np.int64)
    k = 0
    while active.any():
        c = (tc[bi].astype(np.uint64) + np.uint64(k)) & _M32
        c = c.astype(np.uint32)
        if agent == "avoid":
            act = avoid_actions(N, cp.board, cp.heads, cp.dirs, cp.deaths, g, c, c2, seed, noise)
        else:
            act = random_actions(P, g, c, c2, seed)
        if k == 0 and forced:
            f = cand[bi, ai]
            act[ms, np.arange(M)] = np.where(f == 2, -1, f.clip(0, 2)).astype(np.int8)
        rew, term, win = O.tron_step(cp, act)
        length += active
        ret += np.where(active, rew[ms, np.arange(M)].astype(np.int64), 0)
        term = term.astype(bool)
        for p in range(P):
            won[:, p] += active & term & (((win >> p) & 1) != 0)
        stop = term.copy()
        if until == "seat_done":
            stop |= cp.deaths[ms, np.arange(M)] != 0
        if max_steps and k + 1 == max_steps:
            stop[:] = True
        active &= ~stop
        k += 1
    played = np.where(ok_row, R, 0).astype(np.int64)
    rows = lambda x: x.reshape(B, A, R, *x.shape[1:]).sum(axis=2)
    return rows(won), played, rows(length), rows(ret)
