"""Numpy restatement of the scripted avoid agent's contract (include/colosseum_hip.h, crl_tron_sample_avoid) and of the
host loop it defines (sample_avoid + step with auto-reset, plus the crl_tron_stats bookkeeping of a rollout).

Test infrastructure: the stepping itself is the CPU oracle's (``oracle.tron_step``); only the agent and the statistics
are restated here.  ``philox`` is a vectorised Philox4x32-10 (checked against ``oracle.philox4x32`` by the host tests).
"""
import numpy as np

TAG_AVOID = 0x54410000
_M32 = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (broadcast uint32 arrays) under key {seed lo, seed hi}: four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0 & _M32, p1 & _M32, n2 & _M32, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return [x.astype(np.uint32) for x in c]


def threshold(noise):
    """thr = min(2^32, ceil(noise * 2^32)), in 64 bits."""
    return min(1 << 32, int(np.ceil(float(noise) * 4294967296.0)))


def words(g, c, p, seed):
    """W[0..2] of (game g, step counter c, player p): three uint32 arrays of the broadcast shape."""
    w = philox(g, c, p, TAG_AVOID, seed)
    return w[0], w[1], w[2]


def clamped_cell(N, h, d):
    """next_cell(x, y, d, N) with clamping, as a flat index (reference TronGridEnvironment.py:467-481)."""
    h = np.asarray(h, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64) & 3
    x, y = h % N, h // N
    dx = np.array([0, 1, 0, -1])[d]
    dy = np.array([-1, 0, 1, 0])[d]
    return np.clip(y + dy, 0, N - 1) * N + np.clip(x + dx, 0, N - 1)


def decide(N, board, heads, dirs, deaths, g, c, seed, noise):
    """Actions int8 [P, B] (0, +1, -1) of every player; board int8 [B, N*N], heads / dirs / deaths [P, B]; g, c [B].
    Dead players get 0."""
    P, B = heads.shape
    p = np.arange(P, dtype=np.uint64)[:, None]
    w0, w1, w2 = words(np.asarray(g, np.uint64)[None, :], np.asarray(c, np.uint64)[None, :], p, seed)
    thr = threshold(noise)
    rows = np.arange(B)[None, :]
    d = dirs.astype(np.int64)
    probe = lambda off: board[rows, clamped_cell(N, heads, d + off)]
    r_f, r_r, r_l = probe(0), probe(1), probe(3)
    a3 = ((w1.astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int64)
    noisy_act = np.where(a3 == 2, -1, a3)
    left_first = (w2 >> np.uint32(31)) != 0
    first_free = np.where(left_first, r_l, r_r) == 0
    side = np.where(left_first == first_free, -1, 1)
    noisy = w0.astype(np.uint64) < np.uint64(thr)
    act = np.where(noisy, noisy_act, np.where(r_f == 0, 0, side))
    act = np.where(deaths != 0, 0, act)
    return act.astype(np.int8)


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
