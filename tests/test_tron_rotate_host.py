"""The premise of tests/test_gpu_tron_rotate.py, established on the reference side: the rotation of tests/tron_rotate.py is a
symmetry of the contract.  (1) The map itself: four quarter turns are the identity, heads stay on their own cells, and a turn
changes a mid-game state (so the GPU test cannot pass vacuously).  (2) Every restatement the GPU tests are held to gives
bit-identical outputs on the turned state: the two tree searches, the Voronoi areas, info and the territory agent's decision,
the playouts, the avoid agent's decision.  (3) The oracle's step commutes with the turn."""
import functools

import numpy as np
import pytest

from tests import territory_ref as V
from tests import tron_mcts_ref as M
from tests import tron_mcts_territory_ref as T
from tests import tron_ref as TR
from tests.tron_rotate import rotate, rotate_cells, rotate_state

SHAPES = [(7, 3), (9, 5), (13, 4)]
shapes = pytest.mark.parametrize("N,P", SHAPES, ids=["%dx%dp%d" % (n, n, p) for n, p in SHAPES])
agents = pytest.mark.parametrize("agent", ["random", "avoid"])
TURNS = (1, 2, 3)
FIRST_ENV_ID = (1 << 32) + 77
B = 6


@functools.lru_cache(maxsize=None)
def _positions(N, P):
    """(state, seat): B mid-game positions of avoid-agent games at several fill levels, a live seat per game"""
    rng = np.random.default_rng(N * 31 + P)
    st = M.positions(N, P, B, rng)
    seat = np.array([rng.choice(np.flatnonzero(st.deaths[:, b] == 0)) for b in range(B)], np.int8)
    return st, seat


def _parts(st):
    return st.board, st.heads, st.dirs, st.deaths


def _all_equal(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------ 1. the map
@shapes
def test_the_map(N, P):
    st, _ = _positions(N, P)
    assert _all_equal(rotate(N, *_parts(st), k=0), _parts(st)) and _all_equal(rotate(N, *_parts(st), k=4), _parts(st))
    cur = _parts(st)
    for k in TURNS:
        cur = rotate(N, *cur, k=1)
        direct = rotate(N, *_parts(st), k=k)
        assert _all_equal(cur, direct)                            # k turns are one turn k times
        board, heads, dirs, deaths = direct
        assert [a.dtype for a in direct] == [a.dtype for a in _parts(st)] and [a.shape for a in direct] == [a.shape for a in _parts(st)]
        assert (board[np.arange(B)[None, :], heads.astype(np.int64)] == np.arange(1, P + 1)[:, None]).all()   # board[heads[p]] == p + 1
        assert np.array_equal(np.sort(board, axis=1), np.sort(st.board, axis=1)) and np.array_equal(deaths, st.deaths)
        assert (board != st.board).any(axis=1).all() and (dirs != st.dirs).all()       # a turn changes every position
    assert _all_equal(rotate(N, *cur, k=1), _parts(st))
    # the cell map, written out: (x, y) -> (N - 1 - y, x); north becomes east
    assert rotate_cells(N, np.array([0, N - 1, N * N - 1, N * (N - 1), 1 * N + 2])).tolist() == \
        [N - 1, N * N - 1, N * (N - 1), 0, 2 * N + (N - 2)]
    one = rotate(N, np.arange(N * N, dtype=np.int16).reshape(1, N * N), np.zeros((1, 1), np.int16), np.zeros((1, 1), np.int8),
                 np.zeros((1, 1), np.int8))
    assert one[0].dtype == np.int16 and one[0][0, N - 1] == 0 and one[0][0, 0] == N * (N - 1) and one[0][0, N * N - 1] == N - 1
    assert one[1].tolist() == [[N - 1]] and one[2].tolist() == [[1]]


# ------------------------------------------------------------------ 2. the restatements are invariant
@shapes
@agents
def test_playout_search_is_invariant(N, P, agent):
    st, seat = _positions(N, P)
    args = (24, 4, 256, 5, FIRST_ENV_ID, st.tcount, seat, agent, 0.1, 6)
    want = M.tron_mcts(st, *args)
    assert (want[2] > 1).sum() >= B // 2
    for k in TURNS:
        assert _all_equal(M.tron_mcts(rotate_state(st, k), *args), want), k


@shapes
@agents
def test_territory_search_is_invariant(N, P, agent):
    st, seat = _positions(N, P)
    args = (24, 256, 256, 5, FIRST_ENV_ID, st.tcount, seat, agent, 0.1)
    count = T.new_count()
    want = T.tron_mcts_territory(st, *args, count=count)
    assert (want[2] > 1).sum() >= B // 2 and count["flooded"] > 0
    for k in TURNS:
        assert _all_equal(T.tron_mcts_territory(rotate_state(st, k), *args), want), k


@shapes
def test_territory_and_its_agent_are_invariant(N, P):
    """areas and info with nobody forced and with candidates (mixed seats, padding), and the territory agent's decision"""
    st, seat = _positions(N, P)
    rng = np.random.default_rng(N + P)
    seats = rng.integers(-1, P + 1, size=B).astype(np.int8)
    cand = rng.integers(-1, 4, size=(B, 5)).astype(np.int32)
    c3 = np.tile(np.arange(3, dtype=np.int32), (B, 1))
    g = np.arange(B) + 5

    def outputs(s):
        a0, i0 = V.territory(N, *_parts(s))
        a1, i1 = V.territory(N, *_parts(s), seats, cand)
        a2, i2 = V.territory(N, *_parts(s), seat, c3)
        return (a0, i0, a1, i1, a2, i2, V.greedy_action(N, *_parts(s), seat.astype(np.int64)),
                V.decide(N, *_parts(s), g, s.tcount, 0xC0FFEE, 0.1))

    want = outputs(st)
    assert want[0].sum() > 0 and (want[3] == 1).any() and (want[7] != 0).any()
    for k in TURNS:
        assert _all_equal(outputs(rotate_state(st, k)), want), k


@shapes
@agents
@pytest.mark.parametrize("until,max_steps,forced", [("end", 0, True), ("seat_done", 5, False)])
def test_playouts_are_invariant(N, P, agent, until, max_steps, forced):
    st, seat = _positions(N, P)
    cand = np.random.default_rng(P).integers(-1, 4, size=(B, 4)).astype(np.int32) if forced else None
    kw = dict(cand=cand, A=4 if forced else 1, seat=seat, tcount=st.tcount, first_env_id=FIRST_ENV_ID, agent=agent, noise=0.1,
              until=until, max_steps=max_steps)
    want = TR.tron_playout(st, 99, 3, **kw)
    assert (want[1] > 0).any() and want[2].sum() > want[1].sum()          # (playouts longer than one step)
    for k in TURNS:
        assert _all_equal(TR.tron_playout(rotate_state(st, k), 99, 3, **kw), want), k


@shapes
@pytest.mark.parametrize("noise", [0.0, 0.1])
def test_avoid_decision_is_invariant(N, P, noise):
    st, _ = _positions(N, P)
    g = np.arange(B) + 5
    want = TR.decide(N, *_parts(st), g, st.tcount, 77, noise)
    assert (want != 0).any()
    for k in TURNS:
        assert np.array_equal(TR.decide(N, *_parts(rotate_state(st, k)), g, st.tcount, 77, noise), want), k


# ------------------------------------------------------------------ 3. the oracle's step commutes with the turn
@shapes
def test_oracle_step_commutes(N, P):
    """several steps of random actions from mid-game positions, so that walls, trails, heads and edges are hit: the same
    rewards, terminal flags and winners, and the state afterwards is the turned one"""
    from oracle import oracle as O
    st, _ = _positions(N, P)
    rng = np.random.default_rng(N * P)
    for k in TURNS:
        a, b = st.copy(), rotate_state(st, k)
        died = 0
        for _ in range(6):
            act = rng.integers(-1, 2, size=(P, B)).astype(np.int8)
            before = (a.deaths != 0).sum()
            ra, rb = O.tron_step(a, act), O.tron_step(b, act)
            assert _all_equal(ra, rb)
            assert _all_equal(_parts(b), rotate(N, *_parts(a), k=k))
            died += (a.deaths != 0).sum() - before
        assert died > 0
