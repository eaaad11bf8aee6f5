"""A seeded corpus of Blokus positions that uniform random play from the fresh position never reaches: inventories of one
or two pieces (the +15 / +20 last-piece bonuses of ai.py:44-54), players who hold nothing, players whose round-0 corner is
taken, the last plies of real games, finished games, arbitrary boards, and step counters next to the Philox refill and to
2^32.  Built on the CPU oracle alone (oracle.blokus_rollout / blokus_step / blokus_valid / set_board and numpy); no code is
shared with the kernels.  Every family is computed once per process and handed out as a fresh copy (an oracle.BlokusState
with zeroed statistics), so a caller may play on what it gets."""
import os
from functools import lru_cache

import numpy as np

from oracle import oracle as O
from tests.blokus_replay import PIECE_CELLS

CELLS = PIECE_CELLS.astype(np.int64)                                  # cells of piece 0..20; all 21 are worth 89
FULL = (1 << 21) - 1
FIELDS = ("occ", "inv", "score", "round", "to_move")
THREADS = max(1, min(16, os.cpu_count() or 1))
LIST_CAP = 8192                                                        # what oracle.blokus_rollout's own list holds
SEED, FIRST_ENV_ID = 0xB10C, 9000
CORNER_X, CORNER_Y = (0, 19, 0, 19), (0, 0, 19, 19)                    # board.py:50, by player


def held_cells(inv):
    """cells of the pieces in the inventory masks `inv` (any shape)"""
    inv = np.asarray(inv, np.uint32)
    return (((inv[..., None] >> np.arange(21, dtype=np.uint32)) & 1) * CELLS).sum(axis=-1).astype(np.int32)


def clone(st, idx=None):
    """a fresh oracle state holding the games `idx` (default: all) of `st`, statistics and counters zero"""
    idx = np.arange(st.B) if idx is None else np.asarray(idx, np.int64)
    out = O.BlokusState(len(idx))
    for name in FIELDS:
        getattr(out, name)[:] = getattr(st, name)[idx]
    return out


def concat(states):
    """the games of several states in one"""
    out = O.BlokusState(sum(s.B for s in states))
    for name in FIELDS:
        getattr(out, name)[:] = np.concatenate([getattr(s, name) for s in states])
    return out


def counts(st, rnd=None):
    """int32 [B, 4]: the number of legal actions of every player (in round `rnd` instead of the state's own, if given)"""
    if rnd is not None:
        st = clone(st)
        st.round[:] = rnd
    return np.stack([O.blokus_valid(st, player=np.full(st.B, p, np.int8), n_threads=THREADS)[0] for p in range(4)], axis=1)


def _scores_of_inventories(st):
    """Scores are the cells of the pieces no longer held."""
    st.score[:] = 89 - held_cells(st.inv)


# ------------------------------------------------------------------ round 6 boards with crafted inventories
@lru_cache(maxsize=None)
def _base(B):
    st = O.BlokusState(B)
    O.blokus_rollout(st, SEED, FIRST_ENV_ID, 24, n_threads=THREADS)
    assert (st.round == 6).all() and (st.to_move == 0).all() and not st.n_episodes.any()
    return clone(st)


@lru_cache(maxsize=None)
def _tiny(B):
    st = clone(_base(B))
    rng = np.random.default_rng(101)
    kind = rng.integers(0, 4, size=(B, 4))
    other = rng.integers(1, 21, size=(B, 4))                         # any piece but the monomino
    small = rng.integers(1, 9, size=(B, 4))                          # a piece of 2..4 cells
    large = rng.integers(9, 21, size=(B, 4))                         # a pentomino
    small_any = rng.integers(0, 9, size=(B, 4))
    inv = np.where(kind == 0, 1,
          np.where(kind == 1, 1 << other,
          np.where(kind == 2, 1 | (1 << small), (1 << small_any) | (1 << large))))
    st.inv[:] = inv.astype(np.uint32)
    _scores_of_inventories(st)
    return st


def tiny_inventories(B):
    """24 oracle plies from the fresh position (round 6), then every inventory replaced by the monomino alone, one other
    piece, the monomino plus a piece of at most 4 cells, or one small and one large piece."""
    return clone(_tiny(B))


@lru_cache(maxsize=None)
def _all_out(B):
    st = clone(_base(B))
    rng = np.random.default_rng(102)
    full = clone(st)
    full.inv[:] = FULL
    for p in range(4):
        count, ids = O.blokus_valid(full, player=np.full(B, p, np.int8), cap=LIST_CAP, n_threads=THREADS)
        assert count.min() > 0 and count.max() <= LIST_CAP
        for b in range(B):
            pieces = np.unique(ids[b, :count[b]] // 16000)
            piece = 0 if (pieces[0] == 0 and rng.random() < 0.5) else int(rng.choice(pieces))
            st.inv[b, p] = np.uint32(1 << piece)
    _scores_of_inventories(st)
    return st


def all_out(B):
    """The boards of tiny_inventories; every player holds exactly one piece, one that has a legal action: four bonuses are
    possible in one game, and ties at the top."""
    return clone(_all_out(B))


@lru_cache(maxsize=None)
def _empty_handed(B):
    st = clone(_tiny(B))
    rng = np.random.default_rng(103)
    for b in range(B):
        out = rng.choice(4, size=int(rng.integers(1, 4)), replace=False)
        st.inv[b, out] = 0
    st.to_move[:] = rng.integers(0, 4, size=B)
    _scores_of_inventories(st)
    return st


def empty_handed(B):
    """tiny_inventories with one to three players' inventories 0 at entry and any player to move."""
    return clone(_empty_handed(B))


def empty_handed_mover(st):
    """bool [B]: the mover holds nothing"""
    return st.inv[np.arange(st.B), st.to_move & 3] == 0


# ------------------------------------------------------------------ round 0 with a corner taken
@lru_cache(maxsize=None)
def _round0_blocked(B):
    rng = np.random.default_rng(104)
    board = np.zeros((B, 20, 20), np.int8)
    inv = np.full((B, 4), FULL, np.uint32)
    to_move = (np.arange(B) % 4).astype(np.int32)
    blocked = np.zeros((B, 4), bool)
    for b in range(B):
        tm = int(to_move[b])
        blocked[b, (tm + (b // 4) % 4) % 4] = True                    # the mover, the next one, ... in turn
        blocked[b] |= rng.random(4) < 0.2
        short = (b // 16) % 2 == 1                                    # short games: two or three pieces each
        for p in range(4):
            if short:
                inv[b, p] = sum(1 << int(i) for i in rng.choice(21, size=int(rng.integers(2, 4)), replace=False))
            elif rng.random() < 0.5:
                inv[b, p] = np.uint32(rng.integers(1, FULL + 1))
        for p in np.nonzero(blocked[b])[0]:
            board[b, CORNER_Y[p], CORNER_X[p]] = (p + int(rng.integers(1, 4))) % 4 + 1
            # own cells elsewhere: a monomino or a domino inside the player's quadrant, away from the other quadrants
            x = (10 if CORNER_X[p] else 0) + int(rng.integers(3, 7))
            y = (10 if CORNER_Y[p] else 0) + int(rng.integers(3, 7))
            board[b, y, x] = p + 1
            if rng.random() < 0.5:
                board[b, y, x + 1] = p + 1
                inv[b, p] &= ~np.uint32(2)
            elif rng.random() < 0.7:
                inv[b, p] &= ~np.uint32(1)                            # (else: own cells and the inventory untouched)
            if inv[b, p] == 0:
                inv[b, p] = np.uint32(1 << int(rng.integers(2, 21)))
    st = O.BlokusState(B)
    st.set_board(board)
    st.inv[:] = inv
    st.round[:] = 0
    st.to_move[:] = to_move
    _scores_of_inventories(st)
    return st, blocked


def round0_blocked(B, with_blocked=False):
    """Round 0; one or more players' corners are taken by another colour while they hold own cells elsewhere and a full or
    partial inventory (games 16..31, 48..63, ... hold two or three pieces per player: short games); to_move 0..3.  Each
    blocked player has 0 actions in round 0 and more than 0 in round 1.  with_blocked: also the bool [B, 4] of who is."""
    st, blocked = _round0_blocked(B)
    return (clone(st), blocked.copy()) if with_blocked else clone(st)


def round0_short(B):
    """indices of the short games of round0_blocked(B)"""
    return np.nonzero((np.arange(B) // 16) % 2 == 1)[0]


# ------------------------------------------------------------------ the last plies of real games
def _snapshot(st, b):
    return tuple(getattr(st, name)[b].copy() for name in FIELDS)


def _from_snapshots(snaps):
    out = O.BlokusState(len(snaps))
    for k, snap in enumerate(snaps):
        for name, v in zip(FIELDS, snap):
            getattr(out, name)[k] = v
    return out


@lru_cache(maxsize=None)
def _endgames(N=256):
    """N oracle games from the fresh position, uniform random play: the positions before plies 48..66 by what is special
    about them, and every game's final position.  -> {kind: [snapshot]}"""
    st = O.BlokusState(N)
    O.blokus_rollout(st, SEED + 1, FIRST_ENV_ID, 48, n_threads=THREADS)
    assert not st.n_episodes.any()
    rng = np.random.default_rng(105)
    alive = np.ones(N, bool)
    kinds = {"pass2": [], "pass1": [], "ends": [], "finished": []}
    for t in range(48, 120):
        cnt = counts(st)
        count, ids = O.blokus_valid(st, cap=LIST_CAP, n_threads=THREADS)
        assert count.max() <= LIST_CAP
        act = np.full(N, -1, np.int32)
        for b in np.nonzero(alive)[0]:
            m = int(st.to_move[b]) & 3
            c = [int(cnt[b, (m + k) % 4]) for k in range(4)]            # the mover first
            if c[0]:
                act[b] = ids[b, int(rng.integers(0, c[0]))]
            if t > 66:
                continue
            one_piece = c[0] > 0 and len(np.unique(ids[b, :c[0]] // 16000)) == 1
            if sum(c) == 0:
                pass                                                    # (finished: taken below, after its terminal pass)
            elif c[0] == 0 and c[1] == 0:
                kinds["pass2"].append(_snapshot(st, b))                 # two or three movers in a row must pass
            elif c[0] == 0:
                kinds["pass1"].append(_snapshot(st, b))                 # the mover has no action but another player has
            elif c[1] + c[2] + c[3] == 0 and one_piece:
                kinds["ends"].append(_snapshot(st, b))                  # whatever the mover plays ends the game
        _, term, _ = O.blokus_step(st, act, n_threads=THREADS)
        for b in np.nonzero(alive & (term != 0))[0]:
            kinds["finished"].append(_snapshot(st, b))                  # (blokus_step does not reset)
            alive[b] = False
        if not alive.any():
            break
    assert not alive.any()
    return kinds


@lru_cache(maxsize=None)
def _late(B):
    kinds = _endgames()
    order, k = [], 0
    while len(order) < B:
        for name in ("pass2", "ends", "pass1"):
            if k < len(kinds[name]) and len(order) < B:
                order.append(kinds[name][k])
        k += 1
        assert k <= max(len(v) for v in kinds.values()), "not enough late positions"
    return _from_snapshots(order)


def late(B):
    """Positions of real oracle games after 48..66 plies, in turn: two or three movers in a row must pass while the game
    goes on; one ply ends the game; the mover has no action but another player has."""
    return clone(_late(B))


def late_kinds(st):
    """(passes in a row at entry while the game goes on int [B], ends on the next ply bool [B]) of `st`, from the oracle"""
    cnt = counts(st)
    m = st.to_move & 3
    c = np.stack([cnt[np.arange(st.B), (m + k) & 3] for k in range(4)], axis=1)
    goes_on = c.sum(axis=1) > 0
    passes = np.where(goes_on, np.argmax(c > 0, axis=1), 0)
    probe = clone(st)
    count, ids = O.blokus_valid(probe, cap=1)
    _, term, _ = O.blokus_step(probe, np.where(count > 0, ids[:, 0], -1).astype(np.int32))
    return passes, term != 0


@lru_cache(maxsize=None)
def _finished(B):
    st = _from_snapshots(_endgames()["finished"])
    # the reference ends a game on the board BEFORE the last move (:424): the piece just placed may have opened a corner
    # for its owner, and such a final position is not a finished one
    st = clone(st, np.nonzero(counts(st).sum(axis=1) == 0)[0][:B])
    assert st.B == B
    order = np.argsort(st.score[0], kind="stable")
    st.score[0, order[2]] = st.score[0, order[3]]                       # game 0: a tie for the best
    return st


def finished(B):
    """Positions in which nobody has an action (the next ply is the terminal pass); game 0 has a tie for the best score."""
    return clone(_finished(B))


# ------------------------------------------------------------------ boards no game reaches
@lru_cache(maxsize=None)
def _arbitrary(B):
    """the generator of test_blokus_lists_on_arbitrary_boards (tests/test_gpu_soak.py).  A game in which a player has more
    actions than the LIST_CAP entries of the oracle rollout's own list would be drawn again (none is: the largest count at
    entry is about 6,000).  -> (state, the density each board was drawn with)"""
    rng = np.random.default_rng(41)
    keep, dens = [], []
    while sum(s.B for s in keep) < B:
        n = B
        density = rng.choice([0.01, 0.05, 0.15, 0.3, 0.5, 0.7], size=n)
        board = ((rng.random((n, 20, 20)) < density[:, None, None]) * rng.integers(1, 5, (n, 20, 20))).astype(np.int8)
        inv = rng.integers(0, 1 << 21, size=(n, 4)).astype(np.uint32)
        inv[rng.random((n, 4)) < 0.15] = FULL
        inv[rng.random((n, 4)) < 0.05] = 0
        st = O.BlokusState(n)
        st.set_board(board)
        st.inv[:] = inv
        st.round[:] = np.where(rng.random(n) < 0.25, 0, rng.integers(1, 20, n))
        st.to_move[:] = rng.integers(0, 4, n)
        _scores_of_inventories(st)
        ok = np.nonzero(np.maximum(counts(st), counts(st, rnd=1)).max(axis=1) <= LIST_CAP)[0]
        keep.append(clone(st, ok))
        dens.append(density[ok])
    return clone(concat(keep), np.arange(B)), np.concatenate(dens)[:B]


def arbitrary(B, with_density=False):
    """The boards, inventories, rounds and movers of test_blokus_lists_on_arbitrary_boards: random cells of random colours at
    densities from 1 % to 70 %, inventories including 0 and full, round 0 in about a quarter of the games; the sparse boards
    give a player thousands of actions.  with_density: also the density float [B] each board was drawn with."""
    st, density = _arbitrary(B)
    return (clone(st), density.copy()) if with_density else clone(st)


def counters(B):
    """uint32 [B] step counters: 0, 3, 15, 16, 2^32 - 3 and 2^32 - 17 in front, random values behind"""
    front = [0, 3, 15, 16, 2 ** 32 - 3, 2 ** 32 - 17]
    tail = np.random.default_rng(106).integers(0, 2 ** 32, size=max(0, B - len(front)), dtype=np.uint64)
    return np.concatenate([np.array(front, np.uint64), tail])[:B].astype(np.uint32)


FAMILIES = {"tiny_inventories": tiny_inventories, "all_out": all_out, "empty_handed": empty_handed,
            "round0_blocked": round0_blocked, "late": late, "finished": finished, "arbitrary": arbitrary}


def oracle_rollout(st, seed, first_env_id, T):
    """oracle.blokus_rollout(T) on `st`, once it is known that no mover's list outgrows the oracle's own buffer on the way:
    a copy of `st` plays the same T plies one at a time first, the count checked before each"""
    probe = clone(st)
    for name in ("tcount", "tstep"):
        getattr(probe, name)[:] = getattr(st, name)
    for _ in range(T):
        assert int(O.blokus_valid(probe, n_threads=THREADS)[0].max()) <= LIST_CAP
        O.blokus_rollout(probe, seed, first_env_id, 1, n_threads=THREADS)
    O.blokus_rollout(st, seed, first_env_id, T, n_threads=THREADS)


# ------------------------------------------------------------------ what the playout tests start from
PLAYOUT_SEED, PLAYOUT_FIRST_ENV_ID = 31337, 77


@lru_cache(maxsize=None)
def _playout_positions():
    r0 = round0_blocked(64)
    parts = [late(20), tiny_inventories(12), all_out(10), empty_handed(10), clone(r0, round0_short(64)[:8]), finished(7)]
    return concat(parts)


def playout_positions():
    """(state, tcount): 67 positions -- 20 late, 12 tiny_inventories, 10 all_out, 10 empty_handed, 8 short round0_blocked
    and 7 finished -- with `counters`"""
    st = clone(_playout_positions())
    return st, counters(st.B)


@lru_cache(maxsize=None)
def _playout_candidates():
    from tests import blokus_ref as R
    st = _playout_positions()
    rng = np.random.default_rng(107)
    cand = np.full((st.B, 6), -1, np.int64)
    cand[:, 5] = 336000
    for b in range(st.B):
        one = R.blokus_one(st, b)
        legal = R.blokus_list(one)
        member = set(int(i) for i in legal)
        bad = int(rng.integers(0, 336000))
        while bad in member:
            bad = int(rng.integers(0, 336000))
        cand[b, 3] = bad
        if not len(legal):
            continue
        if bin(int(one.inv[0, int(one.to_move[0]) & 3])).count("1") == 1:
            cand[b, 0] = int(rng.choice(legal))                       # the mover's last piece
        for piece in np.unique(legal // 16000):                       # whether the game is over depends on the piece alone
            aid = int(rng.choice(legal[legal // 16000 == piece]))
            probe = R.blokus_one(st, b)
            if O.blokus_step(probe, np.array([aid], np.int32))[1][0]:
                cand[b, 1] = aid
                break
        cand[b, 2] = int(rng.choice(legal))
    return cand


def playout_candidates():
    """int64 [67, 6] for playout_positions: a legal id that plays the mover's last piece (where it has one), a legal id
    after which the game is over (where one exists), another legal id, a dense id that is not legal, -1 and 336000"""
    return _playout_candidates().copy()


def bonus_rows(st, score_sum, R):
    """bool [B, A]: some player's score_sum exceeds R times its score at entry plus the cells it holds -- only a
    last-piece bonus explains that"""
    ceiling = (st.score + held_cells(st.inv)).astype(np.int64) * R
    return (score_sum.astype(np.int64) > ceiling[:, None, :]).any(axis=2)


@lru_cache(maxsize=None)
def _counter_positions():
    st = late(64)
    passes, _ = late_kinds(st)
    return clone(st, np.nonzero(passes >= 1)[0][:16])                # the mover passes: every playout has two plies or more


def counter_cases():
    """(state of 16 late positions, refill bases, wrap bases): with a refill base the step counter reaches a multiple of 16
    at the playout's second ply (the launch starts on an unaligned counter and crosses into the next Philox batch), with a
    wrap base it passes 2^32 there"""
    st = clone(_counter_positions())
    assert st.B == 16
    refill = (np.random.default_rng(108).integers(0, 2 ** 28, size=16, dtype=np.uint64) * 16 + 15).astype(np.uint32)
    refill[1] = 15
    return st, refill, np.full(16, 2 ** 32 - 1, np.uint32)


STRIDE_ROWS = (0, 7, 20, 33, 41, 50, 58, 63, 64, 69)
STRIDE_SEED, STRIDE_FIRST_ENV_ID = 2025, 123456


@lru_cache(maxsize=None)
def _stride_state():
    st = finished(70)
    rng = np.random.default_rng(109)
    for k, b in enumerate(STRIDE_ROWS):
        m, piece = k % 4, 1 + 2 * k                                  # the mover; the piece it holds beside the monomino
        board = np.zeros((1, 20, 20), np.int8)
        board[0, int(rng.integers(7, 13)), int(rng.integers(7, 13))] = m + 1
        one = O.BlokusState(1)
        one.set_board(board)
        st.occ[b] = one.occ[0]
        st.inv[b] = 0
        st.inv[b, m] = np.uint32(1 | (1 << piece))
        st.round[b] = 1 + k
        st.to_move[b] = m
        base = 30 + k
        st.score[b] = (3, 5, 8, 11)
        st.score[b, m] = base
        st.score[b, (m + 1 + k % 3) % 4] = base + 1 + int(CELLS[piece]) + 17   # between the mover's two possible finals
    return st


def stride_state():
    """(state, tcount) of 70 rows: `finished` positions, and in the rows STRIDE_ROWS three players hold nothing while the
    mover holds the monomino and one other piece on an open board.  There the game lasts five plies, and the first draw
    alone decides which piece goes last (+20 or +15) and with it who wins."""
    st = clone(_stride_state())
    return st, counters(st.B)


def stride_expected(st, tcount, R, r_values=None):
    """The outcome sums of R playouts (or of the playouts `r_values`) of every row of stride_state in closed form: (wins
    uint32 [B, 1, 4], played, len_sum uint32 [B, 1], score_sum int32 [B, 1, 4])."""
    from tests import blokus_ref as BR
    from tests import rng_ref as RNG
    r = np.arange(R) if r_values is None else np.asarray(r_values)
    n = len(r)
    B = st.B
    best = st.score.max(axis=1, keepdims=True)
    wins = ((st.score == best) * n).astype(np.uint32)                 # a finished position: one terminal pass
    len_sum = np.full(B, n, np.int64)
    score_sum = st.score.astype(np.int64) * n
    for b in STRIDE_ROWS:
        m = int(st.to_move[b])
        legal = BR.blokus_list(BR.blokus_one(st, b))                  # piece-major: the monomino's actions come first
        n_mono = int((legal // 16000 == 0).sum())
        assert 0 < n_mono < len(legal)
        piece = int(legal[-1] // 16000)
        c0 = int(tcount[b])
        word = RNG.philox(STRIDE_FIRST_ENV_ID + b, c0 >> 2, r, RNG.CRL_TAG_BLOKUS_PLAYOUT, STRIDE_SEED)[c0 & 3]
        mono_first = RNG.mulhi(word, len(legal)) < n_mono             # then the other piece goes last: +15
        k15 = int(mono_first.sum())
        cells = 1 + int(CELLS[piece])
        rival = int(np.argmax(st.score[b]))
        assert st.score[b, m] + cells + 15 < st.score[b, rival] < st.score[b, m] + cells + 20
        wins[b] = 0
        wins[b, m], wins[b, rival] = n - k15, k15
        len_sum[b] = 5 * n
        score_sum[b, m] += n * cells + 15 * k15 + 20 * (n - k15)
    played = np.full((B, 1), n, np.uint32)
    return wins[:, None, :], played, len_sum[:, None].astype(np.uint32), score_sum[:, None, :].astype(np.int32)
