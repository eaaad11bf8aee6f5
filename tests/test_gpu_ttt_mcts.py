"""Batched Monte Carlo tree search on the GPU (crl_ttt_mcts, TTTBatch.mcts / mcts_action): every case bit for bit against
the plain-Python restatement of the header's contract (tests/mcts_ref.py) on all four outputs -- seeded mid-game positions
with finished ones and movers out of range among them, counters that are odd, even and about to wrap, a game id base, every
kernel family, the S at which a tree first selects, trees that run into terminal nodes, the largest trees, every launch
geometry, R across one and several passes -- and the strength of the search learner next to flat Monte Carlo."""
import functools

import numpy as np
import pytest
import torch

from tests import mcts_ref as M
from tests.gpu_util import DEV, first_episodes, np_of as _np, ttt_batch

pytestmark = pytest.mark.gpu

# (dims, K, P, built without the win-mask table)
INSTANCES = [((3, 3), 3, 2, False), ((3, 5), 3, 3, False), ((3, 3, 3), 3, 4, False), ((5, 5), 4, 3, False), ((4, 8), 4, 2, False),
             ((3, 3), 3, 2, True)]
IDS = ["3x3p2", "3x5p3", "3x3x3p4", "5x5k4p3", "4x8k4p2", "3x3p2-no-table"]
inst = pytest.mark.parametrize("dims,K,P,no_table", INSTANCES, ids=IDS)
FIRST_ENV_ID = 77


def _batch(st, first_env_id=FIRST_ENV_ID):
    return ttt_batch(st, first_env_id)


def _same(got, want, what=""):
    for key, w in zip(("visits", "value", "nodes", "best"), want):
        g = _np(got[key])
        g = g if key == "best" else g.view(np.uint32)
        assert np.array_equal(g, w), (what, key, np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:8])    # (the positions)


def _check(st, S, Rn, cexp=256, seed=5, no_table=False, monkeypatch=None, tb=None, out=None):
    """the call on a stepper holding `st` against the restatement; returns the stepper and the output dict"""
    if no_table:
        monkeypatch.setenv("CRL_TTT_NO_WIN_TABLE", "1")
    tb = tb or _batch(st)
    got = tb.mcts(S, Rn, seed, cexp / 256, out=out)
    want = M.ttt_mcts(st, S, Rn, cexp, seed, FIRST_ENV_ID, st.tcount)
    _same(got, want, (st.dims, S, Rn, cexp))
    return tb, got


@functools.lru_cache(maxsize=None)
def _positions(dims, K, P, B, plies=None, plant=True):
    return M.positions(dims, K, P, B, np.random.default_rng(sum(dims) * 11 + P + B), plies=plies, plant=plant)


@functools.lru_cache(maxsize=None)
def _late(dims, K, P, B):
    return M.late_positions(dims, K, P, B, np.random.default_rng(sum(dims) * 13 + P))


# ------------------------------------------------------------------ 1. a ragged batch: more than two waves, not a multiple of 64
@inst
def test_batch_of_130(dims, K, P, no_table, monkeypatch):
    """130 positions (finished ones, movers out of range, tcount odd / even / 2^32 - 3, first_env_id 77); S past the empty
    cells of many of them, so that trees expand, select and meet terminal nodes"""
    st = _positions(dims, K, P, 130)
    n = st.n_cells
    S, Rn = (24, 16) if n <= 16 else (40, 4)
    tb, got = _check(st, S, Rn, no_table=no_table, monkeypatch=monkeypatch)
    nodes = _np(got["nodes"])
    assert (nodes == 0).sum() >= 4 and (nodes > 1).sum() >= 100 and (_np(got["best"]) == -1).sum() == (nodes == 0).sum()
    assert int(st.tcount[2]) == 2 ** 32 - 3


# ------------------------------------------------------------------ 2. the S around the first selection, and B = 1
@inst
def test_simulations_around_the_first_selection(dims, K, P, no_table, monkeypatch):
    """every position four plies old (cells - 4 empty cells): S = 1, S = the empty cells (expansion only: one visit per
    child), S = one more (the first selection)"""
    st = _positions(dims, K, P, 12, plies=4, plant=False)
    empty = st.n_cells - 4
    tb = None
    for S in (1, empty, empty + 1):
        tb, got = _check(st, S, 3, no_table=no_table, monkeypatch=monkeypatch, tb=tb)
        if S == empty:
            assert (_np(got["visits"]).sum(axis=1) == S).all() and (_np(got["visits"]).max(axis=1) == 1).all()
            assert (_np(got["nodes"]) == S + 1).all()


@inst
def test_one_position(dims, K, P, no_table, monkeypatch):
    st = _positions(dims, K, P, 1, plies=3, plant=False)
    _check(st, 20, 16, no_table=no_table, monkeypatch=monkeypatch)


# ------------------------------------------------------------------ 3. trees that run into terminal nodes
@inst
def test_few_empty_cells(dims, K, P, no_table, monkeypatch):
    """S = 64 on positions with at most 4 empty cells: at most 1 + 4 + 12 + 24 + 24 nodes, the leaves terminal and
    revisited"""
    st = _late(dims, K, P, 10)
    tb, got = _check(st, 64, 2, no_table=no_table, monkeypatch=monkeypatch)
    assert (_np(got["nodes"]) <= 65).all() and (_np(got["nodes"]) >= 2).all() and (_np(got["visits"]).sum(axis=1) == 64).all()


# ------------------------------------------------------------------ 4. the largest tree of every instance
@inst
def test_max_simulations(dims, K, P, no_table, monkeypatch):
    st = _positions(dims, K, P, 2, plies=2, plant=False)
    if no_table:
        monkeypatch.setenv("CRL_TTT_NO_WIN_TABLE", "1")
    tb = _batch(st)
    S = tb.mcts_max_simulations
    assert S == M.max_simulations(st.n_cells)
    tb, got = _check(st, S, 1, tb=tb)
    assert (_np(got["nodes"]) > S // 2).all()
    with pytest.raises(ValueError):
        tb.mcts(S + 1, 1)


# ------------------------------------------------------------------ 5. every launch geometry of the 3x3 table instance
@pytest.mark.parametrize("S", [530, 531, 2125, 2126, 2440, 2441])
def test_launch_geometry_edges(S):
    """3x3, 26 bytes a node: 4 waves a workgroup up to 531 nodes, then fewer; the win-mask table fits beside the tree up to
    2,126 nodes, the rank table up to 2,441: the S on either side of each edge"""
    st = _positions((3, 3), 3, 2, 5, plies=1, plant=False)
    _check(st, S, 1, cexp=300)


# ------------------------------------------------------------------ 6. R: one pass, a full one, a second with one live lane, many
@pytest.mark.parametrize("Rn", [1, 16, 64, 65])
@pytest.mark.parametrize("dims,K,P", [((3, 3), 3, 2), ((3, 3, 3), 3, 4)], ids=["3x3p2", "3x3x3p4"])
def test_playouts_per_leaf(dims, K, P, Rn):
    st = _positions(dims, K, P, 20)
    _check(st, 14, Rn)


@pytest.mark.parametrize("dims,K,P", [((3, 3), 3, 2), ((3, 3, 3), 3, 4)], ids=["3x3p2", "3x3x3p4"])
def test_1024_playouts(dims, K, P):
    st = _positions(dims, K, P, 1, plies=2, plant=False)
    _check(st, 2, 1024)


# ------------------------------------------------------------------ 7. the exploration constant
@pytest.mark.parametrize("cexp", [0, 256, 65535])
@pytest.mark.parametrize("dims,K,P", [((3, 3), 3, 2), ((5, 5), 4, 3)], ids=["3x3p2", "5x5k4p3"])
def test_exploration(dims, K, P, cexp):
    st = _positions(dims, K, P, 16, plies=None if P == 2 else 19, plant=False)
    _check(st, 40, 4, cexp=cexp)


# ------------------------------------------------------------------ 8. the wrappers
def test_wrappers_out_reuse_and_read_only_state():
    st = _positions((3, 5), 3, 3, 40)
    tb, got = _check(st, 20, 8)
    before = [t.clone() for t in (tb.occ, tb.winner, tb.to_move, tb.tcount)]
    want = M.ttt_mcts(st, 30, 5, 128, 9, FIRST_ENV_ID, st.tcount)
    again = tb.mcts(30, 5, seed=9, exploration=0.5, out=got)             # a second call on the same stepper, `out` reused
    assert all(again[k] is got[k] for k in got)
    _same(again, want)
    act = tb.mcts_action(30, 5, 9, 0.5, out=got)
    assert act.dtype == torch.int64 and np.array_equal(_np(act), want[3].astype(np.int64))
    fresh = tb.mcts_action(30, 5, seed=9, exploration=0.5)
    assert torch.equal(fresh, act)
    for t, b in zip((tb.occ, tb.winner, tb.to_move, tb.tcount), before):
        assert torch.equal(t, b)                                         # the state and the counters are only read
    assert tb.mcts_max_simulations == 1723


def test_graph_replay():
    """the call captured into a graph and replayed on other positions"""
    st = _positions((3, 3), 3, 2, 70)
    tb = _batch(st)
    out = tb.mcts(16, 4, seed=3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                           # warm-up on a side stream, as torch.cuda.graph wants
        tb.mcts(16, 4, seed=3, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tb.mcts(16, 4, seed=3, out=out)
    other = _positions((3, 3), 3, 2, 70, plies=3, plant=False)
    tb.occ.copy_(torch.from_numpy(other.occ.view(np.int32)))
    tb.winner.copy_(torch.from_numpy(other.winner))
    tb.to_move.copy_(torch.from_numpy(other.to_move))
    tb.tcount.copy_(torch.from_numpy(other.tcount.view(np.int32)))
    for v in out.values():
        v.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    _same(out, M.ttt_mcts(other, 16, 4, 256, 3, FIRST_ENV_ID, other.tcount))


# ------------------------------------------------------------------ 9. strength, through the product
def _first_episode_losses(learner, games, seed):
    """the share of `games` first episodes that the learner at seat 1 loses to the noise-free tactical agent"""
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    env = TicTacToeSinglePlayerVectorEnv((3, 3), 3, 2, games, seat=1, seed=seed, device=DEV, opponent="tactical", noise=0.0)
    env.reset()
    reward, _, _ = first_episodes(env, learner, 5)                       # the learner has at most four plies in a game
    return float((reward < 0).float().mean())


def test_search_learner_loses_at_most_half_as_often_as_flat_monte_carlo():
    """3x3, the learner at seat 1 against the noise-free tactical agent, 2,048 games, first episodes: mcts_action(128, 16)
    beside flat_mc_action(256) (256 playouts per cell: at least the search's budget at every position).  The restatement
    alone gives 0.04 against 0.37 over 100 games at equal budgets (tests/test_ttt_mcts_host.py); measured here: 0.0625
    against 0.333."""
    games = 2048
    search = _first_episode_losses(lambda env, step: env.mcts_action(128, 16, seed=100 + step), games, 21)
    flat = _first_episode_losses(lambda env, step: env.batch.flat_mc_action(256, seed=100 + step), games, 21)
    print("first-episode loss rate over %d games: search %.4f, flat Monte Carlo %.4f" % (games, search, flat))
    assert flat > 0 and search <= 0.5 * flat, (search, flat)
