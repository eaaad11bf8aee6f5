"""numpy restatement of every TicTacToe contract of include/colosseum_hip.h but the tree search (tests/mcts_ref.py):
crl_ttt_sample / _rollout / _step_single / _playout with the random agent, crl_ttt_winning_cells and the same four calls
with the tactical (win-or-block) agent.  Written from the header's words over the CPU oracle's own bindings: the plies are
oracle.ttt_step's, the winning cells come from tests.ttt_probes.has_line on o[q] | 1 << e, the draws from rng_ref.philox.
No code is shared with the kernels.

An agent is a function ``agent(dims, K, P, occ, to_move, seed, g, c, c2, tag) -> int8 [N]`` of N games (occ uint32 [P, N],
to_move [N]) with game ids g, step counters c, third counter words c2 (None = 0) and a Philox tag; ``agent.tag`` and
``agent.playout_tag`` are the tags of its per-step calls and of its playouts.  Each frame (`sample`, `rollout`,
`step_single`, `playout`) is written once, steps all its games in lockstep and takes the agent as a parameter.

Also the positions the host and the GPU tests of the tactical agent share (`positions`): random ones, boards with planted
threats at every turn distance from the mover, empty and full boards; and the exact outcome probabilities of 3x3 positions
under uniform random play.

States are the oracle's TTTState (``tcount`` is the step counter of the draws)."""
import functools

import numpy as np

from oracle import oracle as O
from tests import rng_ref as RNG
from tests import ttt_probes as TP

N_POSITIONS = 203

# decision kinds of a noise-free tactical ply (`kinds`)
OVER, OWN, NEXT, LATER, NONE = "over", "own", "next", "later", "none"


def _as_u32(a):
    return np.asarray(a).astype(np.uint32)


def empties(dims, occ):
    """uint32 [N]: E of every game (occ uint32 [P, N])"""
    return np.uint32(TP.full_mask(dims)) & ~np.bitwise_or.reduce(_as_u32(occ), axis=0)


def _popcount(S):
    return np.array([bin(int(s)).count("1") for s in S], np.uint64)


def _nth_set_bit(S, r):
    """the r[i]-th set bit of S[i], ascending"""
    bits = ((S[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(np.int64)
    return ((np.cumsum(bits, axis=1) == (r[:, None] + 1)) & (bits == 1)).argmax(axis=1)


def _counters(g, c, c2):
    g, c = np.asarray(g, np.uint64), np.asarray(c, np.uint64) & np.uint64(RNG.M32)
    return g, c, (np.zeros(len(g), np.uint64) if c2 is None else np.asarray(c2, np.uint64))


# ------------------------------------------------------------------ the random agent
def random_agent(dims, K, P, occ, to_move, seed, g, c, c2, tag):
    """crl_ttt_sample's rule: word (c >> 1) & 3 of block c >> 3, on odd counters multiplied by n + 1 (mod 2^32), picks the
    mulhi32-th of the n empty cells; -1 on a full board"""
    g, c, c2 = _counters(g, c, c2)
    E = empties(dims, occ)
    n = _popcount(E)
    w = np.choose(((c >> np.uint64(1)) & np.uint64(3)).astype(np.int64), RNG.philox(g, c >> np.uint64(3), c2, tag, seed))
    w = np.where((c & np.uint64(1)) != 0, (w.astype(np.uint64) * (n + np.uint64(1))) & np.uint64(RNG.M32), w)
    return np.where(n == 0, -1, _nth_set_bit(E, RNG.mulhi(w, n))).astype(np.int8)


random_agent.tag, random_agent.playout_tag = RNG.CRL_TAG_TTT, RNG.CRL_TAG_TTT_PLAYOUT


# ------------------------------------------------------------------ the tactical agent
def winning_cells_of(dims, K, marks, E):
    """uint32 [N]: W = {e in E[i] : has_line(marks[i] | 1 << e)} for each pair (marks[i], E[i])"""
    marks, E = _as_u32(marks), _as_u32(E)
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


def draws(seed, g, c, c2=None, tag=RNG.CRL_TAG_TTT_TACTICAL):
    """(u, v) uint64 [N] of the header's step 2 for games g at step counters c (third counter word c2, default 0): words
    2 * (c & 1) and 2 * (c & 1) + 1 of block c >> 1"""
    g, c, c2 = _counters(g, c, c2)
    w = RNG.philox(g, c >> np.uint64(1), c2, tag, seed)
    k = 2 * (c & np.uint64(1)).astype(np.int64)
    return np.choose(k, w).astype(np.uint64), np.choose(k + 1, w).astype(np.uint64)


def moves(dims, K, P, occ, to_move, u, v, noise):
    """The tactical move (steps 1, 3, 4, 5) of N games with draws (u, v): (action int8 [N], distance int [N], S uint32 [N]).
    distance: -2 pass, -1 noisy, i = the set of player (mover + i) mod P was chosen, P = nobody has a winning cell."""
    occ, tm = _as_u32(occ), np.asarray(to_move).astype(np.int64)
    N = occ.shape[1]
    E = empties(dims, occ)
    S = E.copy()
    dist = np.full(N, P, np.int64)
    passing = (tm < 0) | (tm >= P) | (E == 0)
    noisy = ~passing & (u < np.uint64(RNG.threshold(noise)))
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
    action = _nth_set_bit(S, RNG.mulhi(v, _popcount(S)))
    return np.where(passing, -1, action).astype(np.int8), dist, S


def tactical_agent(noise):
    """the win-or-block agent at noise level `noise`"""
    def agent(dims, K, P, occ, to_move, seed, g, c, c2, tag):
        u, v = draws(seed, g, c, c2, tag)
        return moves(dims, K, P, occ, to_move, u, v, noise)[0]
    agent.tag, agent.playout_tag = RNG.CRL_TAG_TTT_TACTICAL, RNG.CRL_TAG_TTT_TACTICAL_PLAYOUT
    return agent


def kinds(st):
    """the decision kind of a noise-free tactical ply on every game of `st`, and the chosen sets: (list of str, S uint32
    [B], E)"""
    zero = np.zeros(st.B, np.uint64)
    _, dist, S = moves(st.dims, st.K, st.P, st.occ, st.to_move, zero, zero, 0.0)
    name = {-2: OVER, 0: OWN, 1: NEXT, st.P: NONE}
    return [name.get(int(d), LATER) for d in dist], S, empties(st.dims, st.occ)


# ------------------------------------------------------------------ the frames
def sample(st, seed, agent, first_env_id=0, advance=True):
    """crl_ttt_sample / _sample_tactical on every game of `st`: int8 [B]; `advance` moves st.tcount on"""
    act = agent(st.dims, st.K, st.P, st.occ, st.to_move, seed, first_env_id + np.arange(st.B), st.tcount, None, agent.tag)
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


def rollout(st, seed, agent, T, first_env_id=0):
    """crl_ttt_rollout / _rollout_tactical (T) on `st` (mutated, statistics included)"""
    for _ in range(T):
        step_auto_reset(st, sample(st, seed, agent, first_env_id))


def results(st):
    """the packed rows of crl_ttt_stats.results: n_episodes, len_sum, draw_count, win_count[P]"""
    return np.stack([st.n_episodes, st.len_sum, st.draw_count] + [st.win_count[p] for p in range(st.P)], axis=1).astype(np.int32)


def step_single(st, seat, learner_action, seed, agent, first_env_id=0, rel_mod=None, policy=None):
    """crl_ttt_step_single / _step_single_tactical on every game of `st` (mutated, tcount included), the games in lockstep.
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
        idx = np.flatnonzero(active & ~learner)
        if len(idx):
            act[idx] = agent(st.dims, st.K, P, st.occ[:, idx], st.to_move[idx], seed, g[idx], st.tcount[idx], None, agent.tag)
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


def playout(st, seed, R, agent, cand=None, A=1, first_env_id=0, tcount=None, rows=None):
    """crl_ttt_playout / _playout_tactical on the oracle state `st` (never written), all playouts in lockstep: (wins uint32
    [B, A, P], played uint32 [B, A], len_sum uint32 [B, A]).  rows: optional iterable of (b, a) to compute (the others stay
    0)."""
    B, P, n = st.B, st.P, st.n_cells
    if cand is None:
        assert A == 1
    else:
        cand = np.asarray(cand, np.int64)
        assert cand.shape == (B, A)
    E = empties(st.dims, st.occ)
    todo = []                                                    # (b, a, first or -1) of the rows that play
    for b, a in (rows if rows is not None else [(b, a) for b in range(B) for a in range(A)]):
        if int(st.winner[b]) >= 0 or int(E[b]) == 0 or not 0 <= int(st.to_move[b]) < P:
            continue                                             # a position that is over skips every row
        first = -1
        if cand is not None:
            first = int(cand[b, a])
            if not (0 <= first < n and (int(E[b]) >> first) & 1):
                continue                                         # not an empty cell: the row is skipped
        todo.append((b, a, first))
    wins, played, len_sum = np.zeros((B, A, P), np.uint32), np.zeros((B, A), np.uint32), np.zeros((B, A), np.uint32)
    if not todo:
        return wins, played, len_sum
    rb, ra, rf = (np.repeat(np.array(col, np.int64), R) for col in zip(*todo))
    rr = np.tile(np.arange(R, dtype=np.int64), len(todo))
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
            act[idx] = agent(st.dims, st.K, P, one.occ[:, idx], one.to_move[idx], seed, first_env_id + rb[idx], c[idx],
                             (ra[idx] << 16) | rr[idx], agent.playout_tag)
            c[idx] = (c[idx] + np.uint64(1)) & np.uint64(RNG.M32)
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


def one_game(st, b):
    """a one-game oracle state holding game b of `st`"""
    one = O.TTTState(st.dims, st.K, st.P, 1)
    one.occ[:, 0] = st.occ[:, b]
    one.winner[0], one.to_move[0] = st.winner[b], st.to_move[b]
    return one


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
