"""Numpy restatement of Tron's scripted agents and of the calls built on them (include/colosseum_hip.h): the avoid agent
(crl_tron_sample_avoid) and the host loop it defines (sample_avoid + step with auto-reset, plus the crl_tron_stats
bookkeeping of a rollout), and crl_tron_playout: R playouts per row (b, a) on private copies of position b, the seat's
forced first action, the random or avoid agent under the playout tags, the stop rules and the four outputs.

Test infrastructure: the stepping itself is the CPU oracle's (``oracle.tron_step``; in a playout all copies at once, copies
that have stopped keep being stepped but are no longer counted); only the agents and the statistics are restated here, over
``rng_ref.philox``.
"""
import numpy as np

from tests import rng_ref as RNG

_POW3 = np.array([1, 3, 9, 27, 81, 243, 729, 2187], np.uint64)
_M32 = np.uint64(RNG.M32)


def words(g, c, p, seed):
    """W[0..2] of (game g, step counter c, player p) of crl_tron_sample_avoid: three uint32 arrays of the broadcast shape."""
    w = RNG.philox(g, c, p, RNG.CRL_TAG_TRON_AVOID, seed)
    return w[0], w[1], w[2]


def clamped_cell(N, h, d):
    """next_cell(x, y, d, N) with clamping, as a flat index (reference TronGridEnvironment.py:467-481)."""
    h = np.asarray(h, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64) & 3
    x, y = h % N, h // N
    dx = np.array([0, 1, 0, -1])[d]
    dy = np.array([-1, 0, 1, 0])[d]
    return np.clip(y + dy, 0, N - 1) * N + np.clip(x + dx, 0, N - 1)


def nonzero(cells):
    """crl_tron_sample_avoid's occupancy test"""
    return cells != 0


def positive(cells):
    """crl_tron_playout's occupancy test"""
    return cells > 0


def decide(N, board, heads, dirs, deaths, g, c, seed, noise, c2=None, tag=RNG.CRL_TAG_TRON_AVOID, occupied=nonzero):
    """Actions int8 [P, B] (0, +1, -1) of the avoid agent for every player; board int8 [B, N*N], heads / dirs / deaths
    [P, B]; g, c [B].  Dead players get 0.  Player p draws from the counter (g, c, p, tag), as crl_tron_sample_avoid does,
    or, given third words c2 [B], from (g, c, c2, tag | p), as the playouts do."""
    P, B = heads.shape
    thr = np.uint64(RNG.threshold(noise))
    rows = np.arange(B)
    occ = occupied(board)
    out = np.zeros((P, B), np.int8)
    for p in range(P):
        third, last = (p, tag) if c2 is None else (c2, tag | p)
        w0, w1, w2, _ = RNG.philox(np.asarray(g, np.uint64), np.asarray(c, np.uint64), third, last, seed)
        d = dirs[p].astype(np.int64)
        probe = lambda off: occ[rows, clamped_cell(N, heads[p], d + off)]
        o_f, o_r, o_l = probe(0), probe(1), probe(3)
        a3 = RNG.mulhi(w1, 3)
        noisy_act = np.where(a3 == 2, -1, a3)
        left_first = (w2 >> np.uint32(31)) != 0
        first_free = ~np.where(left_first, o_l, o_r)
        side = np.where(left_first == first_free, -1, 1)
        act = np.where(w0.astype(np.uint64) < thr, noisy_act, np.where(~o_f, 0, side))
        out[p] = np.where(deaths[p] != 0, 0, act)
    return out


def random_actions(P, g, c, c2, seed):
    """int8 [P, M] of the playouts' random agent at counter c (uint32 [M]) for copies with game ids g and third words c2."""
    out = np.zeros((P, len(g)), np.int8)
    j = c & np.uint32(7)
    for q in range((P + 3) // 4):
        w = RNG.philox(g, c >> np.uint32(3), c2, RNG.CRL_TAG_TRON_PLAYOUT | q, seed)
        word = np.choose((j >> np.uint32(1)).astype(np.int64), w).astype(np.uint64)
        for i in range(4):
            p = 4 * q + i
            if p >= P:
                break
            v = (word * _POW3[(j & np.uint32(1)).astype(np.int64) * 4 + i]) & _M32
            a3 = RNG.mulhi(v, 3)
            out[p] = np.where(a3 == 2, -1, a3)
    return out


class HostLoop:
    """T x (sample_avoid(all players, advance); step(auto_reset)) on the CPU oracle, with the rollout statistics."""

    def __init__(self, N, P, B, start_heads, start_dirs):
        from oracle import oracle as O
        self.O = O
        self.st = O.TronState(N, P, B)
        self.sh = np.asarray(start_heads, np.int16)
        self.sd = np.asarray(start_dirs, np.int8)
        O.tron_reset(self.st, self.sh, self.sd)

    def load(self, board, heads, dirs, deaths):
        st = self.st
        st.board[...] = board
        st.heads[...] = heads
        st.dirs[...] = dirs
        st.deaths[...] = deaths

    def reset_games(self, mask):
        st = self.st
        idx = np.nonzero(mask)[0]
        if idx.size == 0:
            return
        st.board[idx] = 0
        for p in range(st.P):
            st.board[idx, int(self.sh[p])] = p + 1
            st.heads[p, idx] = self.sh[p]
            st.dirs[p, idx] = self.sd[p]
            st.deaths[p, idx] = 0

    def step(self, seed, noise, first_env_id=0):
        st = self.st
        g = np.arange(st.B, dtype=np.uint64) + np.uint64(first_env_id)
        act = decide(st.N, st.board, st.heads, st.dirs, st.deaths, g, st.tcount, seed, noise)
        rew, term, win = self.O.tron_step(st, act)
        st.tcount += 1
        st.tstep += 1
        st.ret_sum += rew.astype(np.int32)
        t = term != 0
        st.n_episodes[t] += 1
        st.len_sum[t] += st.tstep[t]
        st.last_len[t] = st.tstep[t].astype(np.uint16)
        st.last_winners[t] = win[t]
        for p in range(st.P):
            st.win_count[p, t] += ((win[t] >> p) & 1).astype(np.uint32)
        st.tstep[t] = 0
        self.reset_games(t)
        return act, rew, term, win

    def run(self, T, seed, noise, first_env_id=0):
        for _ in range(T):
            self.step(seed, noise, first_env_id)


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
            act = decide(N, cp.board, cp.heads, cp.dirs, cp.deaths, g, c, seed, noise, c2=c2,
                         tag=RNG.CRL_TAG_TRON_AVOID_PLAYOUT, occupied=positive)
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
