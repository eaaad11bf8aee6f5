"""TicTacToe's tactical (win-or-block) agent on the GPU: crl_ttt_winning_cells and crl_ttt_sample_tactical /
_rollout_tactical / _step_single_tactical / _playout_tactical, bit-exact against the numpy restatement of the header's
contract (tests/ttt_ref.py) on its generated positions (planted threats at every turn distance, so that no case
only exercises the fallback: tests/test_ttt_tactical_host.py asserts that on the restatement alone), the identities of
the contract, the random defaults against today's calls, the vector env replayed from a HIP graph, and the strength of
the agent against a uniformly random learner."""
import functools

import numpy as np
import pytest
import torch

from tests import ttt_ref as TR
from tests import ttt_probes as TP
from tests.gpu_util import DEV, np_of as _np, same_ttt_state as _same_state, ttt_batch as _batch, u32_of as _u32

pytestmark = pytest.mark.gpu

ROWS, IDS = TP.INSTANCE_ROWS, TP.INSTANCE_IDS
NOISE = 0.1


def _same_stats(tb, st):
    for name in ("tstep", "n_episodes", "win_count", "draw_count", "len_sum"):
        assert np.array_equal(_u32(getattr(tb, name)), getattr(st, name)), name
    assert np.array_equal(_np(tb.results()), TR.results(st))
    assert np.array_equal(_np(tb.results_from_columns()), TR.results(st))


# ------------------------------------------------------------------ 1. winning cells
@pytest.mark.parametrize("cfg", ROWS, ids=IDS)
def test_winning_cells(cfg):
    st = TR.state_of(cfg)                                            # 203 positions: ragged
    want = TR.winning_cells(st)
    assert (want != 0).any()
    assert np.array_equal(_u32(_batch(st).winning_cells()), want)


@pytest.mark.parametrize("cfg", [((4, 4), 4, 4), ((16,), 6, 7)], ids=["4x4k4p4", "16k6p7"])
def test_without_the_win_table(cfg, monkeypatch):
    """Boards of at most 16 cells on a context without the win-mask table (CRL_TTT_NO_WIN_TABLE makes crl_ttt_create skip
    it): the kernels that play plies compute the win test instead of looking it up; the same sets, moves and games."""
    monkeypatch.setenv("CRL_TTT_NO_WIN_TABLE", "1")
    test_winning_cells(cfg)
    test_sample(cfg, NOISE)
    test_rollout(cfg)
    test_step_single(cfg, True)
    test_playout(*TP.PLAYOUT_CASES[ROWS.index(cfg)])


def _exhaustive(dims, K, P):
    from oracle import oracle as O
    n = TP.n_cells_of(dims)
    if P == 1:
        occ = np.arange(1 << n, dtype=np.uint32)[None, :]
    else:                                                            # every pair of disjoint masks, as base-3 digits
        digits = (np.arange(3 ** n)[:, None] // 3 ** np.arange(n)[None, :]) % 3
        occ = np.stack([TP.pack(digits == 1), TP.pack(digits == 2)])
    st = O.TTTState(dims, K, P, occ.shape[1])
    st.occ[:] = occ
    return st


@pytest.mark.parametrize("dims,K,P", [((3, 3), 3, 2), ((4, 4), 4, 1)], ids=["3x3k3p2", "4x4k4p1"])
@pytest.mark.parametrize("table", [True, False], ids=["table", "no_table"])
def test_winning_cells_exhaustive(dims, K, P, table, monkeypatch):
    """every two-player position of 3x3 (every pair of disjoint masks) and every single-player mask of 4x4, on a context
    with and without the win-mask table"""
    if not table:
        monkeypatch.setenv("CRL_TTT_NO_WIN_TABLE", "1")
    st = _exhaustive(dims, K, P)
    assert np.array_equal(_u32(_batch(st).winning_cells()), TR.winning_cells(st))


WRAP_ROWS = [(cfg, i) for cfg, i in zip(ROWS, IDS) if TP.wrap_runs(cfg[0], cfg[1])]


@pytest.mark.parametrize("cfg", [c for c, _ in WRAP_ROWS], ids=[i for _, i in WRAP_ROWS])
def test_a_wrap_run_is_never_completed(cfg):
    """K cells at a direction's linear stride that leave the board (cells 4, 5, 6 of 3x5): the cell that would complete one
    is no winning cell"""
    from oracle import oracle as O
    dims, K, P = cfg
    runs = TP.wrap_runs(dims, K)
    cases = [(run, c) for run in runs for c in range(TP.n_cells_of(dims)) if (run >> c) & 1]
    st = O.TTTState(dims, K, P, len(cases))
    for b, (run, c) in enumerate(cases):
        st.occ[b % P, b] = run & ~(1 << c)
    got = _u32(_batch(st).winning_cells())
    assert np.array_equal(got, TR.winning_cells(st))
    for b, (run, c) in enumerate(cases):
        assert not (int(got[b % P, b]) >> c) & 1, (hex(run), c)


# ------------------------------------------------------------------ 2. one step of the agent
@pytest.mark.parametrize("noise", [0.0, NOISE, 1.0])
@pytest.mark.parametrize("cfg", ROWS, ids=IDS)
def test_sample(cfg, noise):
    seed, first = 0x5EED0000 + cfg[2], 1 << 33                       # (the game id is the low 32 bits)
    st = TR.state_of(cfg)
    assert {0, 1, 2 ** 32 - 1} <= set(int(c) for c in st.tcount)
    tb = _batch(st, first)
    got = tb.sample_tactical(seed, noise, advance=False)
    torch.cuda.synchronize()
    _same_state(tb, st)                                              # advance=False leaves tcount alone
    want = TR.sample(st, seed, TR.tactical_agent(noise), first, advance=False)
    assert np.array_equal(_np(got), want)
    got = tb.sample_tactical(seed, noise)                            # the same draw, and the counter moves on (2^32 - 1 wraps)
    assert np.array_equal(_np(got), TR.sample(st, seed, TR.tactical_agent(noise), first))
    assert 0 in st.tcount[TR.positions(cfg)["tcount"] == 2 ** 32 - 1]
    _same_state(tb, st)
    assert np.array_equal(_np(tb.sample_tactical(seed, noise)), TR.sample(st, seed, TR.tactical_agent(noise), first))     # the other parity
    _same_state(tb, st)


def test_sample_passes_without_a_mover_or_a_cell():
    cfg = ((3, 5), 3, 3)
    st = TR.state_of(cfg, 70)
    st.to_move[:6] = [3, -1, 127, -128, 4, 3]
    full = TR.empties(st.dims, st.occ) == 0
    assert full.sum() >= 2 and not full[:6].all()
    got = _np(_batch(st).sample_tactical(7, 0.5))
    assert (got[:6] == -1).all() and (got[full] == -1).all() and (got[6:][~full[6:]] >= 0).all()
    assert np.array_equal(got, TR.sample(st, 7, TR.tactical_agent(0.5)))


# ------------------------------------------------------------------ 3. fused rollouts
LAUNCHES = (1, 7, 16)


@functools.lru_cache(maxsize=None)
def _rollout_ref(cfg):
    """the restatement's states after each launch of LAUNCHES from 37 generated positions (made once, read by both tests)"""
    seed, first = 77 + cfg[2], 5000
    st = TR.state_of(cfg, 37)
    snaps = []
    for T in LAUNCHES:
        TR.rollout(st, seed, TR.tactical_agent(NOISE), T, first)
        snaps.append({k: getattr(st, k).copy() for k in ("occ", "winner", "to_move", "tcount", "tstep", "n_episodes",
                                                       "win_count", "draw_count", "len_sum")})
    return seed, first, snaps


def _as_state(cfg, snap):
    from oracle import oracle as O
    st = O.TTTState(*cfg, snap["occ"].shape[1])
    for k, v in snap.items():
        getattr(st, k)[:] = v
    return st


@pytest.mark.parametrize("cfg", ROWS, ids=IDS)
def test_rollout(cfg):
    seed, first, snaps = _rollout_ref(cfg)
    tb = _batch(TR.state_of(cfg, 37), first)
    for T, snap in zip(LAUNCHES, snaps):
        tb.rollout_tactical(T, seed, NOISE)
        torch.cuda.synchronize()
        st = _as_state(cfg, snap)
        _same_state(tb, st)
        _same_stats(tb, st)
    assert int(snaps[-1]["n_episodes"].sum()) > 0


@pytest.mark.parametrize("cfg", ROWS, ids=IDS)
def test_rollout_is_sample_then_step(cfg):
    seed, first, snaps = _rollout_ref(cfg)
    tb = _batch(TR.state_of(cfg, 37), first)
    for _ in range(sum(LAUNCHES)):
        tb.step(tb.sample_tactical(seed, NOISE), auto_reset=True)
    torch.cuda.synchronize()
    _same_state(tb, _as_state(cfg, snaps[-1]))


# ------------------------------------------------------------------ 4. one learner against the tactical agent
def _single_compare(tb, st, seat, act, seed):
    out = tb.step_single(torch.from_numpy(seat).to(DEV), None if act is None else torch.from_numpy(act).to(DEV), seed,
                         opponent="tactical", noise=NOISE)
    reward, done, winners, obs, valid = TR.step_single(st, seat, act, seed, TR.tactical_agent(NOISE))
    torch.cuda.synchronize()
    _same_state(tb, st)
    assert np.array_equal(_np(out["reward"]), reward) and np.array_equal(_np(out["done"]), done)
    assert np.array_equal(_np(out["winners"]), winners)
    assert np.array_equal(_np(out["board"]), obs) and np.array_equal(_u32(out["valid"]), valid)
    return done


@pytest.mark.parametrize("mixed", [False, True], ids=["fixed_seat", "mixed_seats"])
@pytest.mark.parametrize("cfg", ROWS, ids=IDS)
def test_step_single(cfg, mixed):
    P, B, seed = cfg[2], 37, 4321 + cfg[2]
    st = TR.state_of(cfg, B)
    tb = _batch(st)
    rng = np.random.default_rng(P * 10 + mixed)
    seat = (rng.integers(0, P, size=B) if mixed else np.full(B, P - 1)).astype(np.int8)
    n_done = int(_single_compare(tb, st, seat, None, seed).sum())   # learner_action=None: on to the learner's turn
    for _ in range(18):
        n_done += int(_single_compare(tb, st, seat, TP.single_turn_actions(st, rng), seed).sum())
    assert n_done > 0


def _play_as_agent(tb, seat, seed, steps):
    tb.reset()
    out = tb.step_single(seat, None, seed, opponent="tactical", noise=NOISE)
    for _ in range(steps):
        act = tb.sample_tactical(seed, NOISE, advance=False).to(torch.int64)      # the agent's move at the learner's own counter
        out = tb.step_single(seat, act, seed, opponent="tactical", noise=NOISE)
    torch.cuda.synchronize()
    return out


def _check_games_against_rollout(tb, cfg, seed, games, board=None):
    from oracle import oracle as O
    tc, occ, winner, to_move = _u32(tb.tcount), _u32(tb.occ), _np(tb.winner), _np(tb.to_move)
    for g in games:
        ref = O.TTTState(*cfg, 1)
        TR.rollout(ref, seed, TR.tactical_agent(NOISE), int(tc[g]), first_env_id=int(g))
        assert np.array_equal(ref.occ[:, 0], occ[:, g]) and ref.winner[0] == winner[g] and ref.to_move[0] == to_move[g], g
        if board is not None:
            bd = ref.board()[0].astype(np.int16)
            assert np.array_equal(np.where(bd >= 0, (bd - g % cfg[2]) % cfg[2], -1), board[g]), g


@pytest.mark.parametrize("cfg", [((3, 5), 3, 3), ((5, 5), 4, 3), ((3, 3, 3), 3, 4)], ids=["3x5k3p3", "5x5k4p3", "3x3x3k3p4"])
def test_learner_as_agent_is_the_rollout(cfg):
    """a learner that plays the tactical agent's own move reproduces crl_ttt_rollout_tactical, game by game (B = 301: ragged)"""
    from colosseumrl_amd.batched import TTTBatch
    B, seed = 301, 99 + cfg[2]
    tb = TTTBatch(*cfg, B, device=DEV)
    _play_as_agent(tb, torch.from_numpy((np.arange(B) % cfg[2]).astype(np.int8)).to(DEV), seed, 12)
    _check_games_against_rollout(tb, cfg, seed, np.random.default_rng(0).choice(B, size=16, replace=False))


def test_step_single_large_batch():
    from colosseumrl_amd.batched import TTTBatch
    cfg, B, seed = ((3, 3), 3, 2), 262144, 5
    tb = TTTBatch(*cfg, B, device=DEV)
    out = _play_as_agent(tb, torch.from_numpy((np.arange(B) % 2).astype(np.int8)).to(DEV), seed, 9)
    games = np.concatenate([[0, B - 1], np.random.default_rng(1).choice(B, size=46, replace=False)])
    _check_games_against_rollout(tb, cfg, seed, games, _np(out["board"]))


# ------------------------------------------------------------------ 5. playouts
def _playout_check(tb, st, tcount, Rn, cand, seed, first_env_id, noise=NOISE):
    A = 1 if cand is None else cand.shape[1]
    snap = [t.clone() for t in (tb.occ, tb.winner, tb.to_move, tb.tcount)]
    out = tb.playout(Rn, None if cand is None else torch.from_numpy(cand.astype(np.int32)).to(DEV), seed, agent="tactical",
                     noise=noise)
    wins, played, len_sum = TR.playout(st, seed, Rn, TR.tactical_agent(noise), cand=cand, A=A, first_env_id=first_env_id, tcount=tcount)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out["played"]), played)
    assert np.array_equal(_u32(out["wins"]), wins)
    assert np.array_equal(_u32(out["len_sum"]), len_sum)
    assert np.array_equal(_np(out["draws"]), played.astype(np.int64) - wins.sum(axis=2))
    skipped = played == 0                                            # skipped rows hold zeros
    assert not _u32(out["wins"])[skipped].any() and not _u32(out["len_sum"])[skipped].any()
    for a, b in zip(snap, (tb.occ, tb.winner, tb.to_move, tb.tcount)):       # the inputs are read only
        assert torch.equal(a, b)
    return played


def _playout_inputs(cfg):
    st, tcount, rng, first_env_id, seed = TP.playout_case_inputs(cfg)      # 67 positions, counters that wrap
    st.tcount[:] = tcount
    return st, tcount, rng, first_env_id, seed, _batch(st, first_env_id)


@pytest.mark.parametrize("cfg,r_cand,r_none,n_cand", TP.PLAYOUT_CASES, ids=IDS)
def test_playout(cfg, r_cand, r_none, n_cand):
    st, tcount, rng, first_env_id, seed, tb = _playout_inputs(cfg)
    cand = TP.playout_candidates(st.n_cells, st.B, rng, n_cand)      # every cell, -1, n and random values, shuffled
    played = _playout_check(tb, st, tcount, r_cand, cand, seed, first_env_id)
    assert played.any() and not played.all()                         # both played and skipped rows
    played = _playout_check(tb, st, tcount, r_none, None, seed, first_env_id)     # candidates=None
    assert played.any() and not played.all()                         # finished positions are among them


@pytest.mark.parametrize("cfg,Rn", [(((3, 3), 3, 2), 2), (((2, 3), 2, 1), 63), (((3, 5), 3, 3), 64), (((2, 3, 2), 2, 3), 65),
                                    (((2, 2, 2), 2, 2), 130)], ids=["R2", "R63", "R64", "R65", "R130"])
def test_playout_row_lengths(cfg, Rn):
    """rows that are segments inside one wave (2, 63), whole waves (64) and that span waves (65, 130: the atomics)"""
    st, tcount, rng, first_env_id, seed, tb = _playout_inputs(cfg)
    cand = TP.playout_candidates(st.n_cells, st.B, rng, 1)[:, :2]
    assert _playout_check(tb, st, tcount, Rn, cand, seed, first_env_id).any()
    assert _playout_check(tb, st, tcount, Rn, None, seed, first_env_id, noise=0.0).any()


def test_flat_mc_action():
    cfg = ((3, 3), 3, 2)
    st, tcount, rng, first_env_id, seed, tb = _playout_inputs(cfg)
    cells = np.tile(np.arange(9), (st.B, 1))
    wins, played, _ = TR.playout(st, seed, 6, TR.tactical_agent(NOISE), cand=cells, A=9, first_env_id=first_env_id, tcount=tcount)
    want = TR.flat_mc_pick(st, wins, played, cells)
    got = _np(tb.flat_mc_action(6, seed, agent="tactical", noise=NOISE))
    assert np.array_equal(got, want) and (want >= 0).any() and (want < 0).any()


# ------------------------------------------------------------------ 6. the defaults are today's calls
def test_random_defaults_are_the_existing_calls():
    cfg = ((3, 5), 3, 3)
    st = TR.state_of(cfg, 203)
    seat = torch.from_numpy((np.arange(203) % 3).astype(np.int8)).to(DEV)
    act = torch.from_numpy(TP.single_turn_actions(st, np.random.default_rng(3))).to(DEV)
    cand = torch.from_numpy(TP.playout_candidates(15, 203, np.random.default_rng(4)).astype(np.int32)).to(DEV)
    runs = []
    for kw_single, kw_playout in (({}, {}), (dict(opponent="random", noise=0.9), dict(agent="random", noise=0.9))):
        tb = _batch(st)
        got = {"playout." + k: v.clone() for k, v in tb.playout(5, cand, 11, **kw_playout).items()}
        got["pick"] = tb.flat_mc_action(3, 12, **kw_playout).clone()
        got.update(("single." + k, v.clone()) for k, v in tb.step_single(seat, act, 13, **kw_single).items())
        got.update((k, getattr(tb, k).clone()) for k in ("occ", "winner", "to_move", "tcount"))
        runs.append(got)
    torch.cuda.synchronize()
    assert runs[0].keys() == runs[1].keys() and all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    tb = _batch(st)                                                  # ... and the tactical opponent is another one
    tb.step_single(seat, act, 13, opponent="tactical", noise=0.0)
    assert not torch.equal(tb.occ, runs[0]["occ"])


# ------------------------------------------------------------------ 7. the vector env, eager and from a graph
def test_vector_env_graph_replay():
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    from oracle import oracle as O
    cfg, B, seed = ((3, 5), 3, 3), 203, 21
    seat = (np.arange(B) % 3).astype(np.int8)

    def make():
        return TicTacToeSinglePlayerVectorEnv(*cfg, B, seat=torch.from_numpy(seat), seed=seed, device=DEV,
                                              opponent="tactical", noise=NOISE)
    eager, graphed = make(), make()
    st = O.TTTState(*cfg, B)
    _, _, _, obs, _ = TR.step_single(st, seat, None, seed, TR.tactical_agent(NOISE))
    assert np.array_equal(_np(eager.reset()["board"]), obs) and np.array_equal(_np(graphed.reset()["board"]), obs)
    rng = np.random.default_rng(11)
    action = torch.zeros((B,), dtype=torch.int64, device=DEV)

    def step_all(replay):
        a = rng.integers(-2, 16, size=B)
        action.copy_(torch.from_numpy(a))
        e_obs, e_rew, e_done, e_info = eager.step(torch.from_numpy(a).to(DEV))
        res = replay()
        reward, done, winners, obs, valid = TR.step_single(st, seat, a, seed, TR.tactical_agent(NOISE))
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
    assert sum(step_all(replay) for _ in range(10)) > 0
    _same_state(eager.batch, st)
    _same_state(graphed.batch, st)


# ------------------------------------------------------------------ 8. strength
def _learner_win_share(opponent, noise):
    """the share of wins among the finished games of a uniformly random learner (over info['valid']) at seat 0 of 4096 games
    of 3x3, played until every game has finished at least once"""
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    B = 4096
    env = TicTacToeSinglePlayerVectorEnv((3, 3), 3, 2, B, seat=0, seed=2024, device=DEV, opponent=opponent, noise=noise)
    env.reset()
    valid = env.batch.valid_mask()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    bits = 1 << torch.arange(9, device=DEV, dtype=torch.int32)
    seen = torch.zeros(B, dtype=torch.bool, device=DEV)
    wins = finished = 0
    for _ in range(5):                                               # a game lasts at most five learner plies
        free = (valid[:, None] & bits[None, :]) != 0
        score = torch.rand((B, 9), generator=gen, device=DEV).masked_fill(~free, -1.0)
        _, reward, done, info = env.step(score.argmax(dim=1).to(torch.int64))
        wins += int(((done != 0) & (reward == 1)).sum())
        finished += int((done != 0).sum())
        seen |= done != 0
        valid = info["valid"].clone()
    assert bool(seen.all())
    return wins / finished


def test_strength():
    """Bounds from a CPU simulation of the rule (numpy draws, 4096 games x 2 seeds): the learner wins 0.57-0.59 of its games
    against the random agent and 0.06-0.07 against the noise-free tactical one; the binomial deviation at 4096 games is
    below 0.01."""
    rnd, tac = _learner_win_share("random", 0.1), _learner_win_share("tactical", 0.0)
    print("learner win share: random %.4f, tactical %.4f" % (rnd, tac))
    assert rnd >= 0.45, rnd
    assert tac <= 0.15, tac
