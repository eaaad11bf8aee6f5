"""The position corpus of tests/blokus_positions.py on the CPU oracle alone: the conditions that keep the GPU tests of
tests/test_gpu_blokus_endgame.py from passing vacuously (bonuses are reached, movers hold nothing, blocked players come back
in round 1, games end), and the playout restatement of tests/blokus_ref.py against the oracle's own rollout on every
family."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import blokus_positions as P
from tests import blokus_ref as R
from tests import rng_ref as RNG

SEED, FIRST = 0xE27D, 4242


def _play(st, T):
    """T single-ply oracle launches.  -> (plies with +15, plies with +20, bool [B, 4] who collected a bonus in the game's
    first episode, uint8 [B] the first episode's winners mask)"""
    B = st.B
    n15 = n20 = 0
    bonus = np.zeros((B, 4), bool)
    winners = np.zeros(B, np.uint8)
    rows = np.arange(B)
    for _ in range(T):
        m = st.to_move & 3
        inv0, score0 = st.inv[rows, m].copy(), st.score[rows, m].copy()
        first = st.n_episodes == 0
        ends0, sums0, wins0 = st.n_episodes.copy(), st.score_sum.copy(), st.win_count.copy()
        O.blokus_rollout(st, SEED, FIRST, 1, n_threads=P.THREADS)
        ended = st.n_episodes > ends0
        after = np.where(ended, (st.score_sum - sums0)[m, rows], st.score[rows, m])   # (a finished game was reset)
        last = (np.array([bin(int(v)).count("1") for v in inv0]) == 1) & (after > score0)
        extra = after - score0 - P.held_cells(inv0)
        assert set(extra[last].tolist()) <= {15, 20}
        assert ((extra == 20) == (inv0 == 1))[last].all()                # +20 iff the last piece is the monomino
        n15 += int((last & (extra == 15)).sum())
        n20 += int((last & (extra == 20)).sum())
        bonus[rows[last & first], m[last & first]] = True
        mask = sum(((st.win_count - wins0)[p] << p) for p in range(4)).astype(np.uint8)
        winners = np.where(ended & first, mask, winners)
    return n15, n20, bonus, winners


def test_tiny_inventories_reach_both_bonuses_and_end():
    st = P.tiny_inventories(256)
    assert (st.round == 6).all() and np.array_equal(st.score, 89 - P.held_cells(st.inv))
    n15, n20, _, _ = _play(st, 16)
    print("plies with +15:", n15, "with +20:", n20, "games ended:", int((st.n_episodes > 0).sum()),
          "winners:", int(st.win_count.sum()), "episodes:", int(st.n_episodes.sum()))
    assert n15 >= 100 and n20 >= 100
    assert (st.n_episodes >= 1).all()
    assert int(st.win_count.sum()) > int(st.n_episodes.sum())           # ties


def test_all_out_four_bonuses_and_ties():
    st = P.all_out(256)
    assert (np.array([[bin(int(v)).count("1") for v in row] for row in st.inv]) == 1).all()
    assert (P.counts(st) > 0).all()                                     # the one piece held has a legal action
    _, _, bonus, winners = _play(st, 16)
    n_winners = np.array([bin(int(w)).count("1") for w in winners])
    print("games with four bonuses:", int(bonus.all(axis=1).sum()), "with two or more winners:", int((n_winners >= 2).sum()))
    assert bonus.all(axis=1).any() and (n_winners >= 2).any()


def test_empty_handed_movers():
    st = P.empty_handed(256)
    n_empty = (st.inv == 0).sum(axis=1)
    assert n_empty.min() >= 1 and n_empty.max() <= 3 and set(n_empty.tolist()) == {1, 2, 3}
    assert P.empty_handed_mover(st).mean() >= 0.25
    assert P.empty_handed_mover(P.empty_handed(67)).sum() >= 67 // 4


def test_round0_blocked_players_return_in_round_1():
    st, blocked = P.round0_blocked(256, with_blocked=True)
    assert (st.round == 0).all() and set(st.to_move.tolist()) == {0, 1, 2, 3} and blocked.any(axis=1).all()
    assert (P.counts(st)[blocked] == 0).all()
    assert (P.counts(st, rnd=1)[blocked] > 0).all()
    board = st.board
    for p in range(4):                                                  # the corner is another colour's, own cells elsewhere
        assert (board[blocked[:, p], P.CORNER_Y[p], P.CORNER_X[p]] > 0).all()
        assert (board[blocked[:, p], P.CORNER_Y[p], P.CORNER_X[p]] != p + 1).all()
        assert ((board[blocked[:, p]] == p + 1).reshape(-1, 400).sum(axis=1) > 0).all()
    mover_blocked = blocked[np.arange(256), st.to_move]
    next_blocked = blocked[np.arange(256), (st.to_move + 1) & 3]
    assert mover_blocked.sum() >= 32 and next_blocked.sum() >= 32
    assert (P.counts(st)[~blocked] > 0).all()


def test_late_positions_pass_and_end():
    for B in (130, 67):
        st = P.late(B)
        assert st.round.min() >= 12 and (P.counts(st).sum(axis=1) > 0).all()
        passes, ends = P.late_kinds(st)
        print("late(%d): passes in a row" % B, np.bincount(passes).tolist(), "end on the next ply:", int(ends.sum()))
        assert (passes >= 2).sum() >= 10 and ends.sum() >= 10


def test_finished_positions():
    st = P.finished(70)
    assert (P.counts(st) == 0).all()
    assert len(set(map(tuple, st.score.tolist()))) > 60                 # differing scores
    assert (st.score[0] == st.score[0].max()).sum() == 2                # one of them a tie for the best
    _, term, winners = O.blokus_step(st, np.full(70, -1, np.int32))
    assert term.all() and bin(int(winners[0])).count("1") == 2


def test_arbitrary_boards_end_with_empty_inventories():
    for B in (130, 67):                                                 # the sizes the GPU tests take
        st, density = P.arbitrary(B, with_density=True)
        most = np.maximum(P.counts(st), P.counts(st, rnd=1)).max(axis=1)
        print("arbitrary(%d): games by density" % B, {d: int((density == d).sum()) for d in np.unique(density)},
              "with more than 2048 actions:", int((most > 2048).sum()), "the most:", int(most.max()))
        assert set(density.tolist()) == {0.01, 0.05, 0.15, 0.3, 0.5, 0.7}   # every density, the sparse boards with their
        assert (most > 2048).sum() >= 10                                   # long lists included (about 3 games in 10)
        assert most.max() <= P.LIST_CAP
        assert (st.inv == 0).any() and (st.inv == P.FULL).any() and 0.1 < (st.round == 0).mean() < 0.45
    st = P.arbitrary(64)
    P.oracle_rollout(st, SEED, FIRST, 30)
    print("empty inventories after 30 plies:", int((st.inv == 0).sum()), "of", st.inv.size)
    assert (st.inv == 0).any()


def test_counters():
    c = P.counters(67)
    assert c.dtype == np.uint32 and c[:6].tolist() == [0, 3, 15, 16, 2 ** 32 - 3, 2 ** 32 - 17] and len(set(c.tolist())) == 67


@pytest.mark.parametrize("family", list(P.FAMILIES))
def test_restatement_plays_the_oracles_rollout(family):
    """blokus_ref's playout ply loop under the rollout's tag and c2 = 0 leaves the state oracle.blokus_rollout leaves, on a
    dozen games of the family, ply for ply up to each game's first terminal ply, whose outcome the rollout's statistics hold."""
    st = P.FAMILIES[family](67)
    tcount = P.counters(67)
    for b in range(12):
        g, c0 = FIRST + b, int(tcount[b])
        mine, theirs = R.blokus_one(st, b), R.blokus_one(st, b)
        theirs.tcount[0] = c0
        c, plies = c0, 0
        while True:
            mask, _, c = R.blokus_random_plies(mine, SEED, g, c, 0, RNG.CRL_TAG_BLOKUS, max_plies=1)
            plies += 1
            O.blokus_rollout(theirs, SEED, g, 1)
            assert int(theirs.tcount[0]) == c
            if mask is not None:
                break
            for name in P.FIELDS:
                assert np.array_equal(getattr(mine, name), getattr(theirs, name)), (family, b, plies, name)
        assert theirs.n_episodes[0] == 1 and theirs.len_sum[0] == plies, (family, b)
        assert np.array_equal(theirs.score_sum[:, 0], mine.score[0]), (family, b)
        assert sum(int(theirs.win_count[p, 0]) << p for p in range(4)) == mask, (family, b)


def test_endgame_fixture_starts_from_the_corpus(golden):
    """the reference's endgame games (tests/golden/blokus_endgame.npz) start from the states the generator takes from this
    corpus today: a changed corpus asks for `python oracle/gen_golden_blokus.py endgame`"""
    from oracle import gen_golden_blokus as G
    g = golden("blokus_endgame")
    for name, want in zip(("start_board", "start_inv", "start_score", "start_round", "start_player", "family"), G.endgame_starts()):
        assert np.array_equal(g[name], want), name
    assert all(np.issubdtype(v.dtype, np.integer) for v in g.values())


# ------------------------------------------------------------------ the playout cases of the GPU tests
def test_playout_candidates_cover_their_kinds():
    st, _ = P.playout_positions()
    cand = P.playout_candidates()
    assert st.B == 67 and cand.shape == (67, 6)
    over = last = 0
    for b in range(67):
        legal = set(int(i) for i in R.blokus_list(R.blokus_one(st, b)))
        for a in range(3):
            assert cand[b, a] == -1 or int(cand[b, a]) in legal
        assert 0 <= cand[b, 3] < 336000 and int(cand[b, 3]) not in legal
        over += cand[b, 1] >= 0
        last += cand[b, 0] >= 0
    assert over >= 5 and last >= 10 and (cand[:, 4] == -1).all() and (cand[:, 5] == 336000).all()


def test_counter_cases_cross_inside_the_playout():
    """every playout of the counter test has two plies or more, so a base of 15 mod 16 reaches the next Philox batch and a
    base of 2^32 - 1 passes 2^32 inside it"""
    st, refill, wrap = P.counter_cases()
    assert (refill & 15 == 15).all() and (wrap == 2 ** 32 - 1).all()
    for base in (refill, wrap):
        for b in range(st.B):
            for r in range(3):
                _, plies, _ = R.blokus_one_playout(st, b, P.PLAYOUT_SEED, P.PLAYOUT_FIRST_ENV_ID + b, int(base[b]), None, 0, r)
                assert plies >= 2, (b, r)


def test_stride_rows_closed_form():
    """the closed form of the grid-stride test against the restatement, playout by playout, for 64 values of r"""
    st, tcount = P.stride_state()
    assert st.B * 65535 > 4 << 20
    r_values = [0, 1, 2, 65534, 65533, 32768] + np.random.default_rng(3).integers(3, 65533, size=58).tolist()
    both = set()
    for b in list(P.STRIDE_ROWS) + [1, 68]:
        for r in r_values:
            want = P.stride_expected(st, tcount, 65535, r_values=[r])
            mask, plies, score = R.blokus_one_playout(st, b, P.STRIDE_SEED, P.STRIDE_FIRST_ENV_ID + b, int(tcount[b]), None, 0, r)
            assert plies == want[2][b, 0] == (5 if b in P.STRIDE_ROWS else 1)
            assert np.array_equal(score, want[3][b, 0]) and mask == sum(int(want[0][b, 0, p]) << p for p in range(4))
            if b in P.STRIDE_ROWS:
                m = int(st.to_move[b])
                both.add(int(score[m]) - int(st.score[b, m]) - int(P.held_cells(st.inv[b, m])))
    assert both == {15, 20}
    wins, played, len_sum, score_sum = P.stride_expected(st, tcount, 65535)
    assert (played == 65535).all() and (len_sum[list(P.STRIDE_ROWS)] == 5 * 65535).all()
    for b in P.STRIDE_ROWS:                                             # neither piece goes last in every playout
        assert 0 < wins[b, 0, int(st.to_move[b])] < 65535
