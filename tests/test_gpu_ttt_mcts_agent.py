"""The tree search as a seated agent on the GPU (crl_ttt_sample_mcts / _rollout_mcts / _step_single_mcts through TTTBatch
and TicTacToeSinglePlayerVectorEnv): every case bit for bit against the restatement of the header's contract
(tests/mcts_agent_ref.py over the frames of tests/ttt_ref.py) -- fused self-play rollouts with games that end and restart
inside the launch, counters that are odd, even and about to wrap, a game id base, every kernel family, the noise levels
(at noise 1 the tactical agent's own entries), the one-step call next to crl_ttt_mcts, the single-player step with the
search in every other seat, R across one and several passes, every launch geometry, a step replayed from a graph -- and the
strength of the search opponent next to the tactical one."""
import functools

import numpy as np
import pytest
import torch

from tests import mcts_agent_ref as AR
from tests import mcts_ref as M
from tests import ttt_probes as TP
from tests import ttt_ref as TR
from tests.gpu_util import DEV, first_episodes, np_of as _np, same_ttt_state as _same_state, ttt_batch, u32_of as _u32

pytestmark = pytest.mark.gpu

# (dims, K, P, built without the win-mask table): the instances of tests/test_gpu_ttt_mcts.py
INSTANCES = [((3, 3), 3, 2, False), ((3, 5), 3, 3, False), ((3, 3, 3), 3, 4, False), ((5, 5), 4, 3, False), ((4, 8), 4, 2, False),
             ((3, 3), 3, 2, True)]
IDS = ["3x3p2", "3x5p3", "3x3x3p4", "5x5k4p3", "4x8k4p2", "3x3p2-no-table"]
inst = pytest.mark.parametrize("dims,K,P,no_table", INSTANCES, ids=IDS)
FIRST_ENV_ID = 77
STATS = ("tstep", "n_episodes", "win_count", "draw_count", "len_sum")


def _batch(st, no_table=False, monkeypatch=None):
    if no_table:
        monkeypatch.setenv("CRL_TTT_NO_WIN_TABLE", "1")
    return ttt_batch(st, FIRST_ENV_ID)


def _copy(st):
    from oracle import oracle as O
    out = O.TTTState(st.dims, st.K, st.P, st.B)
    for k in ("occ", "winner", "to_move", "tcount") + STATS:
        getattr(out, k)[:] = getattr(st, k)
    return out


def _same_stats(tb, st):
    for name in STATS:
        assert np.array_equal(_u32(getattr(tb, name)), getattr(st, name)), name
    assert np.array_equal(_np(tb.results()), TR.results(st))
    assert np.array_equal(_np(tb.results_from_columns()), TR.results(st))


def _budget(n_cells):
    return (24, 4) if n_cells <= 16 else (40, 2)


@functools.lru_cache(maxsize=None)
def _positions(dims, K, P, B, plies=None):
    """seeded running mid-game positions (nothing planted): tcount 3, 8 and 2^32 - 3 in front"""
    return M.positions(dims, K, P, B, np.random.default_rng(sum(dims) * 7 + P + B), plies=plies, plant=False)


# ------------------------------------------------------------------ 1. fused rollouts: a ragged batch and a single game
T_ROLLOUT, NOISE = 12, 0.1


@functools.lru_cache(maxsize=None)
def _rollout_ref(dims, K, P, B):
    """the restatement after T_ROLLOUT plies from _positions (made once; the table and no-table cases of 3x3 share it)"""
    S, Rn = _budget(TP.n_cells_of(dims))
    st = _copy(_positions(dims, K, P, B))
    TR.rollout(st, 5, AR.mcts_agent(S, Rn, 256, NOISE), T_ROLLOUT, FIRST_ENV_ID)
    return st


@inst
@pytest.mark.parametrize("B", [130, 1])
def test_rollout(dims, K, P, no_table, B, monkeypatch):
    """130 games: three waves past 32 workgroups of four; T = 12 plies of the search agent (noise 0.1) from mid-game
    positions, so that games end and restart inside the launch and searches start from the empty board"""
    S, Rn = _budget(TP.n_cells_of(dims))
    start = _positions(dims, K, P, B)
    assert [int(c) for c in start.tcount[:3]] == [3, 8, 2 ** 32 - 3][:B]
    tb = _batch(start, no_table, monkeypatch)
    tb.rollout_mcts(T_ROLLOUT, S, Rn, 5, 1.0, NOISE)
    torch.cuda.synchronize()
    want = _rollout_ref(dims, K, P, B)
    _same_state(tb, want)
    _same_stats(tb, want)
    if B > 1:
        assert (want.n_episodes > 0).mean() >= 0.25, float((want.n_episodes > 0).mean())     # ended and restarted in the launch
        assert 2 ** 32 - 3 + T_ROLLOUT - 2 ** 32 in [int(c) for c in want.tcount]             # the counter that wrapped


# ------------------------------------------------------------------ 2. the noise levels; noise 1 is the tactical agent at noise 1
@pytest.mark.parametrize("noise", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("no_table", [False, True], ids=["table", "no-table"])
def test_noise_levels(noise, no_table, monkeypatch):
    dims, K, P, B, T, S, Rn, seed = (3, 3), 3, 2, 40, 7, 12, 3, 9
    start = _positions(dims, K, P, B)
    tb = _batch(start, no_table, monkeypatch)
    want = _copy(start)
    got = tb.sample_mcts(S, Rn, seed, 1.0, noise, advance=False)
    assert np.array_equal(_np(got), TR.sample(want, seed, AR.mcts_agent(S, Rn, 256, noise), FIRST_ENV_ID, advance=False))
    tb.rollout_mcts(T, S, Rn, seed, 1.0, noise)
    torch.cuda.synchronize()
    TR.rollout(want, seed, AR.mcts_agent(S, Rn, 256, noise), T, FIRST_ENV_ID)
    _same_state(tb, want)
    _same_stats(tb, want)
    assert int(want.n_episodes.sum()) > 0
    if noise == 1.0:                                     # through the product itself: the tactical entries at noise 1
        other = _batch(start)
        assert torch.equal(other.sample_tactical(seed, 1.0, advance=False), got)
        other.rollout_tactical(T, seed, 1.0)
        torch.cuda.synchronize()
        for name in ("occ", "winner", "to_move", "tcount") + STATS:
            assert torch.equal(getattr(other, name), getattr(tb, name)), name
        assert torch.equal(other.results(), tb.results())


# ------------------------------------------------------------------ 3. one step of the agent
@inst
def test_sample_is_the_searchs_best(dims, K, P, no_table, monkeypatch):
    """noise 0, advance=False: `best` of mcts(...) on running positions, the state untouched; with `advance` only tcount moves"""
    S, Rn = _budget(TP.n_cells_of(dims))
    st = _copy(_positions(dims, K, P, 70))
    tb = _batch(st, no_table, monkeypatch)
    act = tb.sample_mcts(S, Rn, 4, 1.2, advance=False)
    torch.cuda.synchronize()
    _same_state(tb, st)
    best = tb.mcts(S, Rn, 4, 1.2)["best"]
    assert act.dtype == torch.int8 and torch.equal(act.to(torch.int32), best) and bool((best >= 0).all())
    again = tb.sample_mcts(S, Rn, 4, 1.2)
    st.tcount += np.uint32(1)
    assert torch.equal(again, act)
    _same_state(tb, st)
    assert 2 ** 32 - 2 in st.tcount


def test_sample_passes_without_a_mover_or_a_cell():
    st = M.positions((3, 5), 3, 3, 24, np.random.default_rng(6))     # planted: a full board, movers out of range, a recorded winner
    want = TR.sample(_copy(st), 3, AR.mcts_agent(16, 2, 256, 0.0), FIRST_ENV_ID, advance=False)
    got = _np(_batch(st).sample_mcts(16, 2, 3))
    assert np.array_equal(got, want) and (want == -1).sum() == 3 and want[24 - 2] >= 0      # (the winner is not read)


@pytest.mark.parametrize("dims,K,P", [((3, 3), 3, 2), ((3, 3, 3), 3, 4)], ids=["3x3p2", "3x3x3p4"])
def test_rollout_is_sample_then_step(dims, K, P):
    S, Rn = _budget(TP.n_cells_of(dims))
    tb = _batch(_positions(dims, K, P, 130))
    for _ in range(T_ROLLOUT):
        tb.step(tb.sample_mcts(S, Rn, 5, 1.0, NOISE), auto_reset=True)
    torch.cuda.synchronize()
    _same_state(tb, _rollout_ref(dims, K, P, 130))


# ------------------------------------------------------------------ 4. one learner against the search agent
def _single_compare(tb, st, seat, act, seed, agent, out=None, **kw):
    got = tb.step_single(torch.from_numpy(seat).to(DEV), None if act is None else torch.from_numpy(act).to(DEV), seed,
                         out=out, opponent="mcts", **kw)
    reward, done, winners, obs, valid = TR.step_single(st, seat, act, seed, agent, FIRST_ENV_ID)
    torch.cuda.synchronize()
    _same_state(tb, st)
    assert np.array_equal(_np(got["reward"]), reward) and np.array_equal(_np(got["done"]), done)
    assert np.array_equal(_np(got["winners"]), winners)
    assert np.array_equal(_np(got["board"]), obs) and np.array_equal(_u32(got["valid"]), valid)
    return got, done, winners


@inst
def test_step_single(dims, K, P, no_table, monkeypatch):
    """a fresh batch, learner_action=None first; then 6 consecutive steps with learner actions that are empty cells, passes,
    occupied cells and values out of range; seats mixed over the batch (P >= 3: middle seats among them, so that a call plays
    several searches); `out` reused"""
    from oracle import oracle as O
    B, seed, noise = 37, 14 + P, 0.05
    S, Rn = (16, 3) if TP.n_cells_of(dims) <= 16 else (20, 2)
    agent = AR.mcts_agent(S, Rn, 128, noise)
    kw = dict(noise=noise, simulations=S, playouts=Rn, exploration=0.5)
    st = O.TTTState(dims, K, P, B)
    tb = _batch(st, no_table, monkeypatch)
    rng = np.random.default_rng(P * 10 + len(dims))
    seat = (np.arange(B) % P).astype(np.int8)
    assert P < 3 or ((seat > 0) & (seat < P - 1)).any()
    out, _, _ = _single_compare(tb, st, seat, None, seed, agent, **kw)
    assert (st.to_move == seat).all() and (st.tcount == seat).all()          # seat[b] searches opened each game
    own = theirs = reopened = 0
    for _ in range(6):
        act = TP.single_turn_actions(st, rng)
        again, done, winners = _single_compare(tb, st, seat, act, seed, agent, out=out, **kw)
        assert all(again[k] is out[k] for k in ("board", "valid", "done"))
        own += int(((done != 0) & (winners == seat)).sum())                  # only the learner's own ply gives it a line
        theirs += int(((done != 0) & (winners >= 0) & (winners != seat)).sum())
        reopened += int(((done != 0) & (seat > 0)).sum())                    # restarted: an opponent searched the empty board
    if dims == (3, 3):                                                       # (larger boards: test_step_single_ends_on_either_ply)
        assert theirs > 0 and reopened > 0, (own, theirs, reopened)


def test_step_single_ends_on_either_ply():
    """3x3 late positions (at most 4 empty cells) with the learner to move: games end on the learner's ply and on the
    opponent's, and a restarted game at seat 1 is opened by a search from the empty board"""
    dims, K, P, B, seed = (3, 3), 3, 2, 48, 3
    st = M.late_positions(dims, K, P, B, np.random.default_rng(12))
    seat = st.to_move.astype(np.int8).copy()
    tb = _batch(st)
    agent = AR.mcts_agent(24, 4, 256, 0.0)
    rng = np.random.default_rng(1)
    own = theirs = reopened = 0
    for _ in range(3):
        act = TP.single_turn_actions(st, rng)
        before = st.tcount.copy()
        _, done, winners = _single_compare(tb, st, seat, act, seed, agent, simulations=24, playouts=4, noise=0.0)
        plies = (st.tcount - before).astype(np.int64)
        own += int(((done != 0) & (plies == np.where(seat == 0, 1, 2)) & (winners != 1 - seat)).sum())
        theirs += int(((done != 0) & (winners == 1 - seat)).sum())
        reopened += int(((done != 0) & (seat == 1)).sum())
    assert own > 0 and theirs > 0 and reopened > 0, (own, theirs, reopened)


# ------------------------------------------------------------------ 5. R: one lane, a full pass, a second pass with one live lane
@pytest.mark.parametrize("Rn", [1, 64, 65])
def test_playouts_per_leaf(Rn):
    start = _positions((3, 3), 3, 2, 6)
    tb = _batch(start)
    tb.rollout_mcts(3, 10, Rn, 2)
    torch.cuda.synchronize()
    want = _copy(start)
    TR.rollout(want, 2, AR.mcts_agent(10, Rn, 256, 0.0), 3, FIRST_ENV_ID)
    _same_state(tb, want)
    _same_stats(tb, want)


# ------------------------------------------------------------------ 6. every launch geometry (the search's own LDS layout)
@pytest.mark.parametrize("S", [530, 531, 2125, 2126, 2440, 2441])
def test_launch_geometry_edges(S):
    """3x3, 26 bytes a node: 4 waves a workgroup up to 531 nodes, then fewer; the win-mask table fits beside the tree up to
    2,126 nodes, the rank table up to 2,441: the S on either side of each edge, in the rollout and the single-player step"""
    from oracle import oracle as O
    start = _positions((3, 3), 3, 2, 5, 1)
    tb = _batch(start)
    agent = AR.mcts_agent(S, 1, 300, 0.0)
    want = _copy(start)
    tb.rollout_mcts(2, S, 1, 8, 300 / 256)
    torch.cuda.synchronize()
    TR.rollout(want, 8, agent, 2, FIRST_ENV_ID)
    _same_state(tb, want)
    _same_stats(tb, want)
    st = O.TTTState((3, 3), 3, 2, 5)
    tb = _batch(st)
    seat = np.array([1, 0, 1, 1, 0], np.int8)
    kw = dict(simulations=S, playouts=1, exploration=300 / 256, noise=0.0)
    _single_compare(tb, st, seat, None, 8, agent, **kw)


# ------------------------------------------------------------------ 7. the vector env, eager and from a graph
def test_vector_env_graph_replay():
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    from oracle import oracle as O
    cfg, B, seed, S, Rn = ((3, 5), 3, 3), 67, 21, 16, 3
    seat = (np.arange(B) % 3).astype(np.int8)
    agent = AR.mcts_agent(S, Rn, 256, 0.1)

    def make():
        return TicTacToeSinglePlayerVectorEnv(*cfg, B, seat=torch.from_numpy(seat), seed=seed, device=DEV, opponent="mcts",
                                              noise=0.1, simulations=S, playouts=Rn)
    eager, graphed = make(), make()
    st = O.TTTState(*cfg, B)
    _, _, _, obs, _ = TR.step_single(st, seat, None, seed, agent)
    assert np.array_equal(_np(eager.reset()["board"]), obs) and np.array_equal(_np(graphed.reset()["board"]), obs)
    rng = np.random.default_rng(11)
    action = torch.zeros((B,), dtype=torch.int64, device=DEV)

    def step_all(replay):
        a = rng.integers(-2, 16, size=B)
        action.copy_(torch.from_numpy(a))
        e_obs, e_rew, e_done, e_info = eager.step(torch.from_numpy(a).to(DEV))
        res = replay()
        reward, done, winners, obs, valid = TR.step_single(st, seat, a, seed, agent)
        torch.cuda.synchronize()
        for o, rew, dn, info in ((e_obs, e_rew, e_done, e_info), res):
            assert np.array_equal(_np(o["board"]), obs) and np.array_equal(_np(rew), reward) and np.array_equal(_np(dn), done)
            assert np.array_equal(_u32(info["valid"]), valid) and np.array_equal(_np(info["winners"]), winners)
        return int(done.sum())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                       # warm-up on a side stream, as torch.cuda.graph wants
        step_all(lambda: graphed.step(action))
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # one launch: a single linear chain (nothing runs here)
        res = graphed.step(action)

    def replay():
        g.replay()
        return res
    assert sum(step_all(replay) for _ in range(5)) > 0
    _same_state(eager.batch, st)
    _same_state(graphed.batch, st)


# ------------------------------------------------------------------ 8. strength, through the product
def _first_episode_wins(games, seed, **opponent):
    """the share of `games` first episodes that a uniformly random learner at seat 0 of 3x3 wins"""
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    env = TicTacToeSinglePlayerVectorEnv((3, 3), 3, 2, games, seat=0, seed=seed, device=DEV, **opponent)
    env.reset()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    bits = 1 << torch.arange(9, device=DEV, dtype=torch.int32)

    def uniform(env, step):
        free = (env.batch.valid_mask()[:, None] & bits[None, :]) != 0
        return torch.rand((games, 9), generator=gen, device=DEV).masked_fill(~free, -1.0).argmax(dim=1).to(torch.int64)
    reward, _, _ = first_episodes(env, uniform, 5)                   # the learner has at most five plies in a game
    return float((reward > 0).float().mean())


def test_the_search_opponent_is_at_least_twice_as_hard_as_the_tactical_one():
    """3x3, a uniformly random learner at seat 0, 2,048 first episodes: it wins at most half as often against the noise-free
    search opponent (64 simulations x 16 playouts, exploration 1.0) as against the noise-free tactical agent, whose share is
    above 0.  The restatement alone gives 3 against 19 of 200 (the issue's table; tests/test_ttt_mcts_agent_host.py holds the
    same condition): the factor of two is the margin over that ratio of about 6."""
    games = 2048
    tactical = _first_episode_wins(games, 2024, opponent="tactical", noise=0.0)
    search = _first_episode_wins(games, 2024, opponent="mcts", noise=0.0, simulations=64, playouts=16, exploration=1.0)
    print("learner win share over %d first episodes: against tactical %.4f, against the search %.4f" % (games, tactical, search))
    assert tactical > 0 and search <= 0.5 * tactical, (search, tactical)
