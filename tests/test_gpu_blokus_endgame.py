"""The fused Blokus kernels (rollout, playout, step_single, step_observe, sample) started from the positions of
tests/blokus_positions.py, which uniform random play from the fresh position never reaches: the +15 / +20 last-piece
bonuses inside the two ply loops, players who hold nothing, the `dead` cache with a player blocked in round 0, chains of
passes, finished games, arbitrary boards; and the playout at its counter, shape and grid-stride edges and under graph
capture.  Against the CPU oracle and the restatement of tests/blokus_ref.py, bit for bit; tests/test_blokus_positions_host.py
holds the conditions that keep these comparisons from passing vacuously."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import blokus_positions as P
from tests import blokus_ref as R
from tests.gpu_util import blokus_batch, np_of, to_dev, u32_of

pytestmark = pytest.mark.gpu

STATE = ("occ", "inv", "score", "round", "to_move")
STATS = ("tcount", "tstep", "n_episodes", "win_count", "len_sum", "score_sum")


def _same(bb, st, names, where):
    for name in names:
        want = getattr(st, name)
        assert np.array_equal(np_of(getattr(bb, name)).view(want.dtype), want), (name, where)


def _load(bb, st, tcount):
    """other positions into the state tensors of an existing batch"""
    for name in STATE:
        getattr(bb, name).copy_(torch.from_numpy(getattr(st, name).view(np.int32)))
    bb.tcount.copy_(torch.from_numpy(tcount.view(np.int32)))


# ------------------------------------------------------------------ 1. the rollout, per family
@pytest.mark.parametrize("family,B", [("tiny_inventories", 130), ("all_out", 67), ("empty_handed", 130), ("round0_blocked", 130),
                                      ("late", 67), ("finished", 67), ("arbitrary", 130)])
def test_rollout_vs_oracle(family, B):
    """Launches of 1, 5 and 14 plies: each starts with empty `dead` / `can_move` caches, in the middle of a chain of passes
    where the family has them; games end and restart inside them."""
    seed, first = 0xB10C05, 4242
    st = P.FAMILIES[family](B)
    st.tcount[:] = P.counters(B)
    st.tstep[:] = np.where(np.arange(B) % 2 == 1, 3 + np.arange(B), 0)
    bb = blokus_batch(st, first_env_id=first, tcount=st.tcount)
    bb.tstep.copy_(torch.from_numpy(st.tstep.view(np.int32)))
    for T in (1, 5, 14):
        bb.rollout(T, seed)
        P.oracle_rollout(st, seed, first, T)                           # oracle.blokus_rollout(T), its list size checked first
        _same(bb, st, STATE + STATS, (family, T))
        assert torch.equal(bb.results(), bb.results_from_columns())
    if family in ("tiny_inventories", "all_out", "empty_handed", "finished"):
        assert (st.n_episodes >= 1).all()                              # every game ended inside the launches
    if family in ("tiny_inventories", "all_out"):
        assert int(st.score_sum.max()) > 89                            # ... some of them with a bonus


# ------------------------------------------------------------------ 2. the playout against the restatement
def _playout_check(bb, st, tcount, Rn, cand, seed, first_env_id, rows=None, out=None):
    A = 1 if cand is None else cand.shape[1]
    snap = [getattr(bb, name).clone() for name in STATE + ("tcount",)]
    out = bb.playout(Rn, None if cand is None else to_dev(cand.astype(np.int32)), seed, out=out)
    want = R.blokus_playout(st, seed, Rn, cand=cand, A=A, first_env_id=first_env_id, tcount=tcount, rows=rows)
    torch.cuda.synchronize()
    _playout_same(out, want)
    for a, name in zip(snap, STATE + ("tcount",)):                      # the state is only read
        assert torch.equal(a, getattr(bb, name)), name
    return want


def _playout_same(out, want):
    wins, played, len_sum, score_sum = want
    assert np.array_equal(u32_of(out["played"]), played)
    assert np.array_equal(u32_of(out["wins"]), wins)
    assert np.array_equal(u32_of(out["len_sum"]), len_sum)
    assert np.array_equal(np_of(out["score_sum"]), score_sum)
    assert np.array_equal(np_of(out["draws"]), played.astype(np.int64) - wins.sum(axis=2))


def test_playout_against_restatement():
    st, tcount = P.playout_positions()
    seed, first = P.PLAYOUT_SEED, P.PLAYOUT_FIRST_ENV_ID
    bb = blokus_batch(st, first, tcount)
    wins, played, len_sum, score_sum = _playout_check(bb, st, tcount, 5, None, seed, first)
    assert (played == 5).all() and (len_sum[-7:] == 5).all()            # the finished positions: one terminal pass
    assert int(P.bonus_rows(st, score_sum, 5).sum()) >= 20              # rows that only a last-piece bonus explains
    cand = P.playout_candidates()
    wins, played, len_sum, score_sum = _playout_check(bb, st, tcount, 2, cand, seed, first)
    assert not played[:, 3:].any() and played[:, :3].any()
    assert ((len_sum == played) & (played > 0)).any()                   # over after the candidate
    bonus = P.bonus_rows(st, score_sum, 2)
    assert bonus[:, 0].any()                                            # the bonus through the candidate
    assert int(bonus.sum()) >= 20


def test_playout_counters():
    """the Philox refill at an unaligned counter crossed inside the playout, and a counter that passes 2^32 there"""
    st, refill, wrap = P.counter_cases()
    seed, first = P.PLAYOUT_SEED, P.PLAYOUT_FIRST_ENV_ID
    bb = blokus_batch(st, first, refill)
    for base in (refill, wrap):
        bb.tcount.copy_(torch.from_numpy(base.view(np.int32)))
        _, played, len_sum, _ = _playout_check(bb, st, base, 3, None, seed, first)
        assert (len_sum >= 2 * played).all()


def test_playout_shape_edges():
    """A = 65535 (c2 = a << 16 | r at its top; skipped rows cost nothing) and R = 65535 (closed form on finished positions)"""
    seed, first = P.PLAYOUT_SEED, P.PLAYOUT_FIRST_ENV_ID
    every, _ = P.playout_positions()
    has_move = O.blokus_valid(every)[0] > 0
    # the first position with a legal action of late, tiny_inventories, all_out, empty_handed and round0_blocked
    st = P.clone(every, [lo + int(np.argmax(has_move[lo:hi])) for lo, hi in ((0, 20), (20, 32), (32, 42), (42, 52), (52, 60))])
    tcount = P.counters(5)
    A = 65535
    cand = np.full((5, A), -1, np.int64)
    rows = []
    for b in range(5):
        legal = R.blokus_list(R.blokus_one(st, b))
        cand[b, 0], cand[b, A - 1] = legal[0], legal[-1]
        rows += [(b, 0), (b, A - 1)]
    bb = blokus_batch(st, first, tcount)
    _, played, _, _ = _playout_check(bb, st, tcount, 2, cand, seed, first, rows=rows)
    assert int(played.sum()) == 2 * len(rows) and played[rows[-1]] == 2
    st = P.finished(5)
    Rn = 65535
    out = blokus_batch(st, first, tcount).playout(Rn, None, seed)
    torch.cuda.synchronize()
    best = st.score.max(axis=1, keepdims=True)
    want = (((st.score == best) * Rn).astype(np.uint32)[:, None, :], np.full((5, 1), Rn, np.uint32), np.full((5, 1), Rn, np.uint32),
            (st.score * Rn).astype(np.int32)[:, None, :])
    _playout_same(out, want)


def test_playout_grid_stride_loop():
    """70 rows x 65535 playouts: more than the 4 * 2^20 the launch has waves for, so the kernel's loop goes round.  Most
    rows are finished positions; ten are sensitive to r (tests/blokus_positions.py stride_state)."""
    st, tcount = P.stride_state()
    Rn = 65535
    assert st.B * Rn > 4 << 20
    bb = blokus_batch(st, P.STRIDE_FIRST_ENV_ID, tcount)
    out = bb.playout(Rn, None, P.STRIDE_SEED)
    want = P.stride_expected(st, tcount, Rn)
    torch.cuda.synchronize()
    _playout_same(out, want)


def test_playout_graph_replay():
    """the call captured into a graph and replayed on other positions"""
    seed, first = P.PLAYOUT_SEED, P.PLAYOUT_FIRST_ENV_ID
    late = P.late(130)
    st, other = P.clone(late, np.arange(70)), P.clone(late, np.arange(60, 130))
    tcount, tcount2 = P.counters(70), P.counters(130)[60:].copy()
    bb = blokus_batch(st, first, tcount)
    out = bb.playout(2, None, seed)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                          # warm-up on a side stream, as torch.cuda.graph wants
        bb.playout(2, None, seed, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bb.playout(2, None, seed, out=out)
    _load(bb, other, tcount2)
    for v in out.values():
        v.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    _playout_same(out, R.blokus_playout(other, seed, 2, first_env_id=first, tcount=tcount2))


# ------------------------------------------------------------------ 3. one learner against the random agent
SINGLE_FAMILIES = ("tiny_inventories", "empty_handed", "round0_blocked")
N_SHORT = 27


def _single_positions(family):
    """34 positions; of round0_blocked the first N_SHORT are short games (at most three pieces per player: at most 12
    placements with at most three passes between two of them, so over within 48 plies), the others hold far more"""
    if family == "round0_blocked":
        return P.clone(P.round0_blocked(64), np.concatenate([P.round0_short(64)[:27], np.arange(7)]))
    return P.FAMILIES[family](34)


@pytest.mark.parametrize("rank", [False, True], ids=["id", "rank"])
@pytest.mark.parametrize("family", SINGLE_FAMILIES)
def test_step_single_against_restatement(family, rank):
    """12 calls (16 from round 0: 60 plies or more), seats mixed: the learner plays a legal action of its own -- its last
    piece where it holds one -- through the end of the games and their restart."""
    seed, first = 4321, 55
    st = _single_positions(family)
    B = st.B
    assert B % 4 != 0
    st.tcount[:] = P.counters(B)
    bb = blokus_batch(st, first_env_id=first, tcount=st.tcount)
    rng = np.random.default_rng(11)
    seat = rng.integers(0, 4, size=B).astype(np.int8)
    n_done, n_last, calls = np.zeros(B, np.int64), 0, 16 if family == "round0_blocked" else 12
    for call in range(calls):
        act = np.full(B, -1, np.int64)
        for b in range(B):
            one = R.blokus_one(st, b)
            if call == 0 or (int(one.to_move[0]) & 3) != seat[b]:
                continue                                              # (the first call only advances to the learner's turn)
            ids = R.blokus_list(one)
            if len(ids):
                k = int(rng.integers(0, len(ids)))
                act[b] = k if rank else int(ids[k])
                n_last += bin(int(one.inv[0, seat[b]])).count("1") == 1
        learner = None if call == 0 else act
        out = bb.step_single(to_dev(seat), None if learner is None else to_dev(learner), seed, rank=rank)
        reward, done, winners, n_valid, ob, op, osc = R.blokus_step_single(st, seat, learner, seed, first_env_id=first, rank=rank)
        torch.cuda.synchronize()
        _same(bb, st, STATE + ("tcount",), (family, call))
        for name, want in (("reward", reward), ("done", done), ("winners", winners), ("n_valid", n_valid), ("board", ob),
                           ("pieces", op), ("score", osc)):
            assert np.array_equal(np_of(out[name]), want), (name, family, call)
        assert (reward >= 0).all()
        n_done += done
    ended = n_done[:N_SHORT] if family == "round0_blocked" else n_done
    assert (ended >= 1).all()                                          # the games ended, and went on after their restart
    assert n_last >= 10                                                # learners played their last piece


def _oracle_random_ply(st, seed, first_env_id):
    """the random agent's ply on every game of `st` at its step counter (restarting finished games), from the oracle's list
    and step -> (action, reward, terminal, winners)"""
    count, ids = O.blokus_valid(st, cap=P.LIST_CAP, n_threads=P.THREADS)
    assert count.max() <= P.LIST_CAP
    act = np.array([int(ids[b, R.blokus_draw_rank(seed, first_env_id + b, int(st.tcount[b]), int(count[b]))]) if count[b] else -1
                    for b in range(st.B)], np.int32)
    reward, term, winners = O.blokus_step(st, act, n_threads=P.THREADS)
    st.tcount += np.uint32(1)
    fresh = O.BlokusState(st.B)
    for name in STATE:
        getattr(st, name)[term != 0] = getattr(fresh, name)[term != 0]
    return act, reward, term, winners


@pytest.mark.parametrize("family", SINGLE_FAMILIES)
def test_step_observe_and_sample_vs_oracle(family):
    """12 plies (48 from round 0) of the kernels' own random agent: sample(advance=False) names the action
    step_observe(None) then plays"""
    seed, first = 977, 300
    st = _single_positions(family)
    B = st.B
    st.tcount[:] = P.counters(B)
    bb = blokus_batch(st, first_env_id=first, tcount=st.tcount)
    n_done = np.zeros(B, np.int64)
    for ply in range(48 if family == "round0_blocked" else 12):
        sampled = bb.sample(seed, advance=False)
        out = bb.step_observe(None, seed=seed, auto_reset=True)
        act, reward, term, winners = _oracle_random_ply(st, seed, first)
        torch.cuda.synchronize()
        assert np.array_equal(np_of(sampled), act), (family, ply)
        _same(bb, st, STATE + ("tcount",), (family, ply))
        assert np.array_equal(np_of(out["reward"]), reward) and np.array_equal(np_of(out["terminal"]), term), (family, ply)
        assert np.array_equal(np_of(out["winners"]), winners), (family, ply)
        mover = st.to_move.astype(np.int8)
        ob, op, osc = O.blokus_observe(st, mover)
        assert np.array_equal(np_of(out["n_valid"]), O.blokus_valid(st)[0]) and np.array_equal(np_of(out["player"]).reshape(-1), mover)
        assert np.array_equal(np_of(out["board"]), ob) and np.array_equal(np_of(out["pieces"]), op)
        assert np.array_equal(np_of(out["score"]), osc), (family, ply)
        n_done += term
    assert (n_done[:N_SHORT] >= 1).all() if family == "round0_blocked" else (n_done >= 1).all()
