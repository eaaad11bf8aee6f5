"""numpy restatement of TicTacToe's tactical (win-or-block) agent -- crl_ttt_winning_cells and crl_ttt_sample_tactical /
_rollout_tactical / _step_single_tactical / _playout_tactical (include/colosseum_hip.h) -- written from the header's words:
the winning cells come from tests.ttt_probes.has_line on o[q] | 1 << e (one call per (game, player) over all its empty
cells; many games at once are the same call on the concatenated masks), the draws from oracle.philox4x32, the plies from
oracle.ttt_step.  No code is shared with the kernels.

Also the positions the host and the GPU tests share (`positions`): random ones, boards with planted threats at every turn
distance from the mover, empty and full boards.

States are the oracle's TTTState (``tcount`` is the step counter of the draws)."""
import functools
import math

import numpy as np

from oracle import oracle as O
from tests import ttt_probes as TP

TAG = 0x54630000                           # CRL_TAG_TTT_TACTICAL
TAG_PLAYOUT = 0x54430000                   # CRL_TAG_TTT_TACTICAL_PLAYOUT
M32 = 0xFFFFFFFF
N_POSITIONS = 203

# decision kinds of a noise-free ply (`kinds`)
OVER, OWN, NEXT, LATER, NONE = "over", "own", "next", "later", "none"


def threshold(noise):
    """thr of the header's step 3: min(2^32, ceil(noise * 2^32))"""
    return min(1 << 32, math.ceil(noise * 4294967296.0))


def _key(seed):
    return [seed & M32, (seed >> 32) & M32]


def _u32(a):
    return np.asarray(a).astype(np.uint32)


def empties(dims, occ):
    """uint32 [N]: E of every game (occ uint32 [P, N])"""
    return np.uint32(TP.full_mask(dims)) & ~np.bitwise_or.reduce(_u32(occ), axis=0)


def winning_cells_of(dims, K, marks, E):
    """uint32 [N]: W = {e in E[i] : has_line(marks[i] | 1 << e)} for each pair (marks[i], E[i])"""
    marks, E = _u32(marks), _u32(E)
    n = TP.n_cells_of(dims)
    game, cell = np.nonzero((E[:, None] >> np.arange(n, dtype=np.uint32)[None, :]) & np.uint32(1))
    W = np.zeros(len(marks), np.uint32)
    if len(game):
        bit = np.uint32(1) << cell.astype(np.uint32)
        won = TP.has_line(dims, K, marks[game] | bit)
        np.bitwise_or.at(W, game[won], bit[won])
    return W


def winning_cells(st):
    """crl_ttt_winning_cells: uint32 [P, B]"""
    E = empties(st.dims, st.occ)
    return np.stack([winning_cells_of(st.dims, st.K, st.occ[q], E) for q in range(st.P)])


def draws(seed, g, c, c2=None, tag=TAG):
    """(u, v) uint64 [N] of the header's step 2 for games g at step counters c (third counter word c2, default 0)"""
    g, c = np.asarray(g, np.uint64), np.asarray(c, np.uint64)
    c2 = np.zeros(len(g), np.uint64) if c2 is None else np.asarray(c2, np.uint64)
    u, v = np.zeros(len(g), np.uint64), np.zeros(len(g), np.uint64)
    key = _key(seed)
    for i in range(len(g)):
        w = O.philox4x32([int(g[i]) & M32, (int(c[i]) & M32) >> 1, int(c2[i]) & M32, tag], key)
        k = 2 * (int(c[i]) & 1)
        u[i], v[i] = int(w[k]), int(w[k + 1])
    return u, v


def _nth_set_bit(S, r):
    """the r[i]-th set bit of S[i], ascending"""
    bits = ((S[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(np.int64)
    return ((np.cumsum(bits, axis=1) == (r[:, None] + 1)) & (bits == 1)).argmax(axis=1)


def moves(dims, K, P, occ, to_move, u, v, noise):
    """The tactical move (steps 1, 3, 4, 5) of N games with draws (u, v): (action int8 [N], distance int [N], S uint32 [N]).
    distance: -2 pass, -1 noisy, i = the set of player (mover + i) mod P was chosen, P = nobody has a winning cell."""
    occ, tm = _u32(occ), np.asarray(to_move).astype(np.int64)
    N = occ.shape[1]
    E = empties(dims, occ)
    S = E.copy()
    dist = np.full(N, P, np.int64)
    passing = (tm < 0) | (tm >= P) | (E == 0)
    noisy = ~passing & (u < np.uint64(threshold(noise)))
    dist[noisy], dist[passing] = -1, -2
    pending = ~passing & ~noisy
    for i in range(P):
        idx = np.flatnonzero(pending)
        if len(idx) == 0:
            break
        q = (tm[idx] + i) % P
        W = winning_cells_of(dims, K, occ[q, idx], E[idx])
        hit = idx[W != 0]
        S[hit], dist[hit], pending[hit] = W[W != 0], i, False
    count = np.array([bin(int(s)).count("1") for s in S], np.uint64)
    action = _nth_set_bit(S, ((v * count) >> np.uint64(32)).astype(np.int64))
    return np.where(passing, -1, action).astype(np.int8), dist, S


def kinds(st):
    """the decision kind of a noise-free ply on every game of `st`, and the chosen sets: (list of str, S uint32 [B], E)"""
    zero = np.zeros(st.B, np.uint64)
    _, dist, S = moves(st.dims, st.K, st.P, st.occ, st.to_move, zero, zero, 0.0)
    name = {-2: OVER, 0: OWN, 1: NEXT, st.P: NONE}
    return [name.get(int(d), LATER) for d in dist], S, empties(st.dims, st.occ)


def sample(st, seed, noise, first_env_id=0, advance=True):
    """crl_ttt_sample_tactical on every game of `st`: int8 [B]; `advance` moves st.tcount on"""
    u, v = draws(seed, first_env_id + np.arange(st.B), st.tcount)
    act, _, _ = moves(st.dims, st.K, st.P, st.occ, st.to_move, u, v, noise)
    if advance:
        st.tcount += np.uint32(1)
    return act


def step_auto_reset(st, act):
    """crl_ttt_step with CRL_STEP_AUTO_RESET and the crl_ttt_stats bookkeeping of a rollout ply (tcount apart)"""
    reward, term, ws = O.ttt_step(st, act)
    st.tstep += np.uint32(1)
    over = term != 0
    st.n_episodes[over] += np.uint32(1)
    st.len_sum[over] += st.tstep[over]
    st.draw_count[over & (ws < 0)] += np.uint32(1)
    for p in range(st.P):
        st.win_count[p, over & (ws == p)] += np.uint32(1)
    st.occ[:, over] = 0
    st.winner[over], st.to_move[over], st.tstep[over] = -1, 0, 0
    return reward, term, ws


def rollout(st, seed, noise, T, first_env_id=0):
    """crl_ttt_rollout_tactical(T) on `st` (mutated, statistics included)"""
    for _ in range(T):
        step_auto_reset(st, sample(st, seed, noise, first_env_id))


def results(st):
    """the packed rows of crl_ttt_stats.results: n_episodes, len_sum, draw_count, win_count[P]"""
    return np.stack([st.n_episodes, st.len_sum, st.draw_count] + [st.win_count[p] for p in range(st.P)], axis=1).astype(np.int32)


def step_single(st, seat, learner_action, seed, noise, first_env_id=0, rel_mod=None, policy=None):
    """crl_ttt_step_single_tactical on every game of `st` (mutated, tcount included), the games in lockstep.
    learner_action int64 [B] or None; `policy(st)` (instead) returns int64 [B] learner actions for the current states.
    Returns (reward int8, done uint8, winners int8, obs int8 [B, cells], valid uint32)."""
    P, B, n = st.P, st.B, st.n_cells
    rel_mod = rel_mod or P
    s = np.asarray(seat, np.int64) % P
    reward, done, winners = np.zeros(B, np.int8), np.zeros(B, np.uint8), np.full(B, -1, np.int8)
    learner = np.full(B, learner_action is not None or policy is not None) & (st.to_move == s)
    opp = np.zeros(B, np.int64)
    g = first_env_id + np.arange(B)
    while True:
        active = learner | ((st.to_move != s) & (opp < 2 * (P - 1)))
        if not active.any():
            break
        act = np.full(B, -1, np.int64)
        if learner.any():
            v = np.asarray(policy(st) if policy is not None else learner_action, np.int64)
            act[learner] = np.where((v >= -1) & (v < n), v, -1)[learner]
        agent = active & ~learner
        idx = np.flatnonzero(agent)
        if len(idx):
            u, w = draws(seed, g[idx], st.tcount[idx])
            act[idx], _, _ = moves(st.dims, st.K, P, st.occ[:, idx], st.to_move[idx], u, w, noise)
            opp[idx] += 1
        learner[:] = False
        before = (st.occ.copy(), st.winner.copy(), st.to_move.copy())
        _, term, ws = O.ttt_step(st, act.astype(np.int8))
        idle = ~active                                           # games that wait at the learner's turn play no ply
        st.occ[:, idle], st.winner[idle], st.to_move[idle] = before[0][:, idle], before[1][idle], before[2][idle]
        st.tcount[active] += np.uint32(1)
        over = active & (term != 0)
        done[over], winners[over] = 1, ws[over]
        reward[over] = np.where(ws[over] < 0, 0, np.where(ws[over] == s[over], 1, -1))
        st.occ[:, over] = 0
        st.winner[over], st.to_move[over] = -1, 0
    obs = st.board().astype(np.int16)
    obs = np.where(obs >= 0, (obs - s[:, None]) % rel_mod, -1).astype(np.int8)
    return reward, done, winners, obs, empties(st.dims, st.occ)


def playout(st, seed, R, noise, cand=None, A=1, first_env_id=0, tcount=None):
    """crl_ttt_playout_tactical on the oracle state `st` (never written), all playouts in lockstep: (wins uint32 [B, A, P],
    played uint32 [B, A], len_sum uint32 [B, A])."""
    B, P, n = st.B, st.P, st.n_cells
    E = empties(st.dims, st.occ)
    rows = []                                                    # (b, a, first or -1) of the rows that play
    for b in range(B):
        if int(st.winner[b]) >= 0 or int(E[b]) == 0 or not 0 <= int(st.to_move[b]) < P:
            continue                                             # a position that is over skips every row
        for a in range(A):
            first = -1
            if cand is not None:
                first = int(cand[b][a])
                if not (0 <= first < n and (int(E[b]) >> first) & 1):
                    continue                                     # not an empty cell: the row is skipped
            rows.append((b, a, first))
    wins, played, len_sum = np.zeros((B, A, P), np.uint32), np.zeros((B, A), np.uint32), np.zeros((B, A), np.uint32)
    if not rows:
        return wins, played, len_sum
    rb, ra, rf = (np.repeat(np.array(col, np.int64), R) for col in zip(*rows))
    rr = np.tile(np.arange(R, dtype=np.int64), len(rows))
    N = len(rb)
    one = O.TTTState(st.dims, st.K, P, N)
    one.occ[:], one.winner[:], one.to_move[:] = st.occ[:, rb], st.winner[rb], st.to_move[rb]
    c = (np.zeros(N, np.uint64) if tcount is None else np.asarray(tcount, np.uint64)[rb])
    plies, won = np.zeros(N, np.int64), np.full(N, -1, np.int64)
    alive = np.ones(N, bool)
    first_ply = cand is not None
    while alive.any():
        idx = np.flatnonzero(alive)
        act = np.full(N, -1, np.int64)
        if first_ply:                                            # the candidate ply: no draw
            act[:] = rf
        else:
            u, v = draws(seed, first_env_id + rb[idx], c[idx], (ra[idx] << 16) | rr[idx], TAG_PLAYOUT)
            act[idx], _, _ = moves(st.dims, st.K, P, one.occ[:, idx], one.to_move[idx], u, v, noise)
            c[idx] = (c[idx] + np.uint64(1)) & np.uint64(M32)
        _, term, ws = O.ttt_step(one, act.astype(np.int8))       # (a finished playout's further plies are never read)
        plies[idx] += 1
        ended = alive & (term != 0)
        won[ended] = ws[ended]
        alive &= term == 0
        first_ply = False
    for p in range(P):
        np.add.at(wins[:, :, p], (rb, ra), (won == p).astype(np.uint32))
    np.add.at(len_sum, (rb, ra), plies.astype(np.uint32))
    played[rb, ra] = R
    return wins, played, len_sum


def flat_mc_pick(st, wins, played, cells):
    """TTTBatch.flat_mc_action's pick from playout counts over the candidate cells `cells` [B, A]: the cell of the greatest
    2 * wins + draws of the mover among the played rows (ties: the lowest column), -1 where none was played"""
    mover = np.clip(st.to_move.astype(np.int64), 0, st.P - 1)
    mine = np.take_along_axis(wins.astype(np.int64), mover[:, None, None], axis=2)[:, :, 0]
    draws_ = played.astype(np.int64) - wins.astype(np.int64).sum(axis=2)
    value = np.where(played > 0, 2 * mine + draws_, -1)
    best = value.argmax(axis=1)
    pick = np.take_along_axis(np.asarray(cells, np.int64), best[:, None], axis=1)[:, 0]
    return np.where(played.max(axis=1) > 0, pick, -1)


# ------------------------------------------------------------------ the positions the host and GPU tests share
def _scatter(rng, n, P, players, free, density):
    """uint32 [P]: every cell of the mask `free` taken with probability `density` by a random player of `players`"""
    occ = np.zeros(P, np.uint32)
    for cell in range(n):
        if (free >> cell) & 1 and rng.random() < density:
            occ[int(rng.choice(players))] |= np.uint32(1 << cell)
    return occ


def _planted(dims, K, P, rng, distance, second, everyone):
    """One position with a threat of the player `distance` turns behind the mover: that player holds a line of
    TP.line_masks but one cell (with `second`, two lines but one cell each), other marks are scattered off those cells --
    over every player (`everyone`), or only over the players at that turn distance or later, so that nobody before holds
    a winning cell."""
    n, full = TP.n_cells_of(dims), TP.full_mask(dims)
    lines = TP.line_masks(dims, K)
    mover = int(rng.integers(0, P))
    q = (mover + distance) % P
    marks, holes = 0, 0
    for _ in range(2 if second else 1):
        line = int(lines[int(rng.integers(0, len(lines)))])
        free = [cell for cell in range(n) if (line >> cell) & 1 and not (marks >> cell) & 1]
        if not free:
            continue
        hole = int(rng.choice(free))
        if (holes | (1 << hole)) & (marks | (line & ~(1 << hole))):
            continue                                             # the second line would fill the first one's hole
        marks |= line & ~(1 << hole)
        holes |= 1 << hole
    players = list(range(P)) if everyone else [(mover + d) % P for d in range(distance, P)]
    occ = _scatter(rng, n, P, players, full & ~marks & ~holes, rng.choice([0.0, 0.15, 0.4]))
    occ[q] |= np.uint32(marks)
    return occ, mover


@functools.lru_cache(maxsize=None)
def positions(cfg, B=N_POSITIONS):
    """dict(occ uint32 [P, B], winner int8 [B], to_move int8 [B], tcount uint32 [B]) for a row (dims, K, P) of
    TP.INSTANCE_ROWS, made once per process and read-only: random positions (TP.random_positions), planted threats at
    every turn distance 0..P-1 from the mover, double threats, empty boards (nobody can have a winning cell) and full
    ones (the pass), shuffled; the counters hold 0, odd and even values and 2^32 - 1."""
    dims, K, P = cfg
    rng = np.random.default_rng(sum(dims) * 131 + K * 17 + P)
    n, full = TP.n_cells_of(dims), TP.full_mask(dims)
    n_rand, n_empty, n_full, n_double = 55, 9, 10, 33
    n_single = B - n_rand - n_empty - n_full - n_double
    rnd = TP.random_positions(dims, K, P, n_rand, rng)
    occ, winner, to_move = [rnd.occ], [rnd.winner], [rnd.to_move]

    def add(o, w, tm):
        occ.append(np.asarray(o, np.uint32).reshape(P, 1))
        winner.append(np.array([w], np.int8))
        to_move.append(np.array([tm], np.int8))
    for i in range(n_single + n_double):
        o, tm = _planted(dims, K, P, rng, i % P, i >= n_single, everyone=(i // P) % 3 == 2)
        add(o, -1, tm)
    for _ in range(n_empty):
        add(np.zeros(P, np.uint32), -1, rng.integers(0, P))
    for _ in range(n_full):
        add(_scatter(rng, n, P, list(range(P)), full, 1.0), -1, rng.integers(0, P))
    order = rng.permutation(B)
    tcount = rng.integers(0, 2 ** 32, size=B, dtype=np.uint64).astype(np.uint32)
    tcount[:6] = [0, 1, 2, 2 ** 32 - 1, 2 ** 32 - 2, 7]
    out = dict(occ=np.concatenate(occ, axis=1)[:, order], winner=np.concatenate(winner)[order],
               to_move=np.concatenate(to_move)[order], tcount=tcount)
    for v in out.values():
        v.setflags(write=False)
    return out


def state_of(cfg, B=N_POSITIONS):
    """a fresh oracle state holding B of the positions of `cfg`, spread evenly over all of them"""
    dims, K, P = cfg
    pos = positions(cfg)
    pick = (np.arange(B) * N_POSITIONS) // B
    st = O.TTTState(dims, K, P, B)
    st.occ[:], st.winner[:], st.to_move[:], st.tcount[:] = pos["occ"][:, pick], pos["winner"][pick], pos["to_move"][pick], pos["tcount"][pick]
    return st
