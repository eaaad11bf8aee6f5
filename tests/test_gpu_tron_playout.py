"""Batched Tron playouts on the GPU (crl_tron_playout): bit-exact against the numpy restatement of the header's contract
(tests/tron_ref.py) on ragged batches of mid-game positions over board sizes, player counts, both agents, both
stop modes and step caps; outcome counts of a tiny board against exact probabilities; read-only inputs, overwritten
outputs, determinism, graph replay, lane indices past 2^31; flat Monte Carlo in TronSinglePlayerVectorEnv against a
random and an avoid learner."""
import math

import numpy as np
import pytest
import torch

from tests import test_tron_playout_host as H
from tests import tron_ref as TR
from tests.gpu_util import DEV, first_episodes, np_of as _np, tron_put

pytestmark = pytest.mark.gpu


def _positions(N, P, B, seed):
    """B mid-game positions from random-agent rollouts (auto-reset, so the games are at different steps), copied to an
    oracle state; a few get dead players, and some are finished (fewer than two alive)."""
    from colosseumrl_amd.batched import TronBatch
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    tb = TronBatch(N, P, B, device=DEV)
    tb.reset()
    tb.rollout(int(rng.integers(3, 3 * N)), seed)
    st = O.TronState(N, P, B)
    st.board[:], st.heads[:], st.dirs[:], st.deaths[:] = _np(tb.board), _np(tb.heads), _np(tb.dirs), _np(tb.deaths)
    if P >= 2:
        for b in rng.choice(B, size=max(1, B // 6), replace=False):     # finished: only player 0 alive
            for p in range(1, P):
                st.deaths[p, b] = st.deaths[p, b] or p + 1
    return tb, st


def _upload(tb, st, tcount, first_env_id):
    tron_put(tb, st.board, st.heads, st.dirs, st.deaths)
    tb.tcount.copy_(torch.from_numpy(tcount.view(np.int32)))
    tb.first_env_id = first_env_id


CASES = [  # N, P, agent, noise, until, max_steps, forced first action
    (5, 2, "random", 0.1, "end", 0, True),
    (19, 4, "random", 0.1, "end", 0, True),
    (19, 4, "avoid", 0.1, "seat_done", 0, True),
    (20, 3, "avoid", 0.0, "end", 0, True),
    (21, 4, "avoid", 1.0, "end", 7, True),
    (40, 4, "avoid", 0.1, "end", 0, False),
    (40, 6, "random", 0.1, "seat_done", 0, True),
    (64, 8, "avoid", 0.1, "seat_done", 0, True),
    (64, 2, "random", 0.1, "end", 3, False),
    (150, 4, "avoid", 0.1, "end", 40, True),
    (181, 1, "random", 0.1, "end", 0, True),
    (7, 1, "avoid", 0.0, "end", 0, False),
    (12, 8, "random", 0.1, "end", 0, True),
    # the remaining tron_playout_kernel<P, AVOID> instances: random P = 3, 5, 7 and avoid P = 2, 5, 6, 7
    (13, 3, "random", 0.1, "end", 0, True),
    (21, 5, "random", 0.1, "seat_done", 0, False),
    (33, 7, "random", 0.1, "end", 0, True),
    (15, 2, "avoid", 0.1, "end", 0, True),
    (20, 5, "avoid", 0.1, "seat_done", 0, False),
    (24, 6, "avoid", 0.3, "end", 0, True),
    (16, 7, "avoid", 0.1, "end", 0, False),
    # the launch geometry's edges: 64 | 65 bitboard words (45 | 46: 256 -> 64 threads) and 512 | 513 (128 | 129: 64 -> 32
    # lanes per wave; 128 KiB of opt-in LDS at 128)
    (45, 4, "random", 0.1, "end", 0, True),
    (46, 4, "avoid", 0.5, "end", 0, False),
    (128, 4, "random", 0.1, "seat_done", 0, False),
    (129, 4, "avoid", 0.5, "end", 60, True),
]


@pytest.mark.parametrize("case", CASES, ids=["N%d_P%d_%s_%g_%s_cap%d_%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "cand" if c[6] else "none")
                                             for c in CASES])
def test_against_restatement(case):
    _check_against_restatement(case)


def _check_against_restatement(case, B=23, Rn=5, A=4, dead_seat=True):
    """B positions, A candidate columns (the last one padding) of Rn playouts each: every output against the restatement."""
    N, P, agent, noise, until, max_steps, forced = case
    seed = 1234 + N * 8 + P
    rng = np.random.default_rng(N * 100 + P)
    tb, st = _positions(N, P, B, seed)
    tcount = (np.uint32(0xFFFFFFF0) + rng.integers(0, 40, size=B).astype(np.uint32)).astype(np.uint32)   # wraps past 2^32
    first_env_id = (1 << 32) - 7
    _upload(tb, st, tcount, first_env_id)
    seat = rng.integers(0, P, size=B).astype(np.int8)
    seat[0], seat[1] = -1, P                                   # out of range: skipped
    if P >= 2 and dead_seat:
        seat[2] = 1
        st.deaths[1, 2] = st.deaths[1, 2] or 1                 # a dead seat: skipped
        tb.deaths.copy_(torch.from_numpy(st.deaths))
    if forced:
        cand = rng.integers(0, 3, size=(B, A)).astype(np.int32)
        cand[:, A - 1] = rng.choice([-1, 3, 7, 2], size=B)      # padding / invalid values skip their rows
    else:
        cand, A = None, 1
    snap = [t.clone() for t in (tb.board, tb.heads, tb.dirs, tb.deaths, tb.tcount)]
    seat_t = torch.from_numpy(seat).to(DEV)
    cand_t = None if cand is None else torch.from_numpy(cand).to(DEV)
    out = tb.playout(Rn, cand_t, seed, agent=agent, noise=noise, seat=seat_t, until=until, max_steps=max_steps)
    torch.cuda.synchronize()
    for x, y in zip(snap, (tb.board, tb.heads, tb.dirs, tb.deaths, tb.tcount)):
        assert torch.equal(x, y)                               # inputs are read only
    w, p, l, r = TR.tron_playout(st, seed, Rn, cand=cand, A=A, seat=seat, tcount=tcount, first_env_id=first_env_id,
                                 agent=agent, noise=noise, until=until, max_steps=max_steps)
    assert (p > 0).any()
    assert np.array_equal(_np(out["played"]), p)
    assert np.array_equal(_np(out["wins"]), w)
    assert np.array_equal(_np(out["len_sum"]), l)
    assert np.array_equal(_np(out["ret_sum"]), r)
    return p


def test_exact_outcome_probabilities():
    """N = 4, P = 2, random agent: counts of 40,000 playouts per row against the exact probabilities (z <= 5)."""
    N, P, Rn, seed = 4, 2, 40000, 77
    st = H._positions(N, P, 3, [0, 1, 2], seed=4)
    from colosseumrl_amd.batched import TronBatch
    tb = TronBatch(N, P, 3, device=DEV)
    _upload(tb, st, np.array([0, 9, 0xFFFFFFFF], np.uint32), 5)
    cand = torch.tensor([[0, 1, 2]] * 3, dtype=torch.int32, device=DEV)
    out = tb.playout(Rn, cand, seed)
    wins, played = _np(out["wins"]), _np(out["played"])
    assert (played == Rn).all()
    for b in range(3):
        for a in range(3):
            ex = H._exact(N, P, st.board[b], st.heads[:, b], st.dirs[:, b], st.deaths[:, b], first=(0, 1, -1)[a])
            for m in (0, 1, 2):
                pq = ex.get(m, 0.0)
                n = int(Rn - wins[b, a].sum()) if m == 0 else int(wins[b, a, m - 1])
                sigma = math.sqrt(Rn * pq * (1 - pq))
                assert abs(n - Rn * pq) <= 5 * sigma + 1, (b, a, m, n, Rn * pq)


def test_outputs_overwritten_and_skipped_rows_zero():
    tb, st = _positions(19, 4, 64, 3)
    _upload(tb, st, np.zeros(64, np.uint32), 0)
    cand = torch.tensor([[0, 1, 2, -1]] * 64, dtype=torch.int32, device=DEV)
    out = {k: torch.full(s, 12345, dtype=torch.int32, device=DEV) for k, s in
           (("wins", (64, 4, 4)), ("played", (64, 4)), ("len_sum", (64, 4)), ("ret_sum", (64, 4)))}
    tb.playout(100, cand, 1, agent="avoid", out=out)      # R = 100: rows span waves (atomics onto zeroed outputs)
    first = {k: v.clone() for k, v in out.items()}
    tb.playout(100, cand, 1, agent="avoid", out=out)
    for k in out:
        assert torch.equal(out[k], first[k])                  # overwritten, not accumulated
        assert (out[k][:, 3] == 0).all()                      # the -1 column is skipped
    finished = torch.from_numpy(((st.deaths != 0).sum(axis=0) >= 3) | (st.deaths[0] != 0)).to(DEV)   # (seat 0)
    assert (out["played"][finished] == 0).all() and (out["played"][~finished, :3] == 100).all()
    w, p, l, r = TR.tron_playout(st, 1, 100, cand=cand.cpu().numpy(), A=4, agent="avoid")
    assert np.array_equal(_np(out["wins"]), w) and np.array_equal(_np(out["ret_sum"]), r)


def test_determinism_and_graph_replay():
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    B, Rn, steps = 512, 16, 6

    def eager():
        env = TronSinglePlayerVectorEnv(15, 4, B, noise=0.1, seed=3, device=DEV)
        env.reset()
        hist = []
        for _ in range(steps):
            a = env.flat_mc_action(Rn, seed=21)
            obs, reward, done, _ = env.step(a)
            hist.append((a.clone(), obs["board"].clone(), reward.clone(), done.clone()))
        return hist

    ref = eager()
    for x, y in zip(ref, eager()):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    env = TronSinglePlayerVectorEnv(15, 4, B, noise=0.1, seed=3, device=DEV)
    env.reset()
    po = env.batch.playout(Rn, torch.zeros((B, 3), dtype=torch.int32, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside the capture (lazy buffers; the state is only read)
        env.flat_mc_action(Rn, seed=21, out=po)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a = env.flat_mc_action(Rn, seed=21, out=po)
        obs, reward, done, _ = env.step(a)
    for k in range(steps):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, ref[k][0]) and torch.equal(obs["board"], ref[k][1])
        assert torch.equal(reward, ref[k][2]) and torch.equal(done, ref[k][3])
    from colosseumrl_amd.batched import TronBatch
    tb = TronBatch(19, 4, 256, device=DEV)
    x = tb.playout(64, seed=1)["wins"].clone()
    assert torch.equal(x, tb.playout(64, seed=1)["wins"])
    assert not torch.equal(x, tb.playout(64, seed=2)["wins"])


def test_lane_index_past_2_31():
    """P = 1: every playout is one terminal step, so B * R > 2^31 lanes are cheap; two rows checked bit-exact."""
    from colosseumrl_amd.batched import TronBatch
    from oracle import oracle as O
    N, B, Rn, seed = 6, 65536, 40000, 8
    assert B * Rn > 2 ** 31
    tb = TronBatch(N, 1, B, device=DEV)
    tb.reset()
    tb.rollout(2, seed)                                     # (a mix of positions)
    out = tb.playout(Rn, None, seed)
    played, wins, lens, rets = (_np(out[k]) for k in ("played", "wins", "len_sum", "ret_sum"))
    assert (played == Rn).all() and (lens == Rn).all()
    assert np.array_equal(rets[:, 0], 10 * wins[:, 0, 0] - (Rn - wins[:, 0, 0]))
    for b in (B - 1, 60000):
        assert b * Rn >= 2 ** 31
        one = O.TronState(N, 1, 1)
        one.board[:] = _np(tb.board)[b:b + 1]
        one.heads[:], one.dirs[:], one.deaths[:] = (_np(t)[:, b:b + 1] for t in (tb.heads, tb.dirs, tb.deaths))
        w, p, l, r = TR.tron_playout(one, seed, Rn, tcount=_np(tb.tcount)[b:b + 1].view(np.uint32), first_env_id=b)
        assert wins[b, 0, 0] == w[0, 0, 0] and rets[b, 0] == r[0, 0]


def _first_episode(policy, B=1024, seed=5, max_t=300):
    """mean first-episode return, steps survived and win rate of a learner in TronSinglePlayerVectorEnv(15, 4, noise 0.1)"""
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    env = TronSinglePlayerVectorEnv(15, 4, B, noise=0.1, seed=seed, device=DEV)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(seed)
    reward, ret, steps = first_episodes(env, lambda env, t: policy(env, t, gen), max_t)
    won = reward == 10                                     # +10: the surviving winner, on the step that ends the game
    return ret.double().mean().item(), steps.double().mean().item(), won.double().mean().item()


def _random_policy(env, t, gen):
    return torch.randint(0, 3, (env.num_envs,), device=DEV, generator=gen)


def _avoid_policy(env, t, gen):
    act = env.batch.sample_avoid(99, env.noise, players=[0], advance=False)[0].to(torch.int64)
    return torch.where(act < 0, 2, act)


def _flat_mc_policy(env, t, gen):
    return env.flat_mc_action(32, seed=1000 + t)


def test_flat_mc_beats_random_learner():
    mc = _first_episode(_flat_mc_policy)
    rnd = _first_episode(_random_policy)
    avd = _first_episode(_avoid_policy)
    print("\nfirst episode (return, steps, win rate): flat MC %s  random %s  avoid %s" % (mc, rnd, avd))
    assert mc[0] >= rnd[0] + 10.0 and mc[1] >= 2 * rnd[1], (mc, rnd)
    assert mc[0] >= avd[0] - 2.0, (mc, avd)                # reported; expected to beat the avoid learner too
