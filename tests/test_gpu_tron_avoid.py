"""The scripted avoid agent on the GPU: crl_tron_sample_avoid against games the reference's own SimpleAvoidAgent played
(tests/golden/tron_avoid_*.npz), crl_tron_rollout_avoid against the two-call loop and the numpy + CPU-oracle loop, and
TronSinglePlayerVectorEnv against a host replay of the same contract (also replayed from a HIP graph)."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import tron_ref
from tests.gpu_util import TRON_STATS as STATS, tron_put as _put, tron_state as _state, tron_stats as _stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "tron_avoid_*.npz")))


def _tb(N, P, B, **kw):
    from colosseumrl_amd.batched import TronBatch
    return TronBatch(N, P, B, device="cuda:0", **kw)


def _load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_sample_avoid_matches_reference_games(path):
    r = _load(path)
    N, P, S, seed = int(r["N"]), int(r["P"]), len(r["c"]), int(r["seed"])
    noise = int(r["noise_num"]) / int(r["noise_den"])
    tb = _tb(N, P, S)
    _put(tb, r["board"], r["heads"].T, r["dirs"].T, r["deaths"].T)
    tb.tcount.copy_(torch.from_numpy(r["c"].astype(np.int32)))
    board0 = tb.board.clone()
    a1 = tb.sample_avoid(seed, noise, advance=False)
    a2 = tb.sample_avoid(seed, noise, advance=True)         # equal inputs, equal outputs
    torch.cuda.synchronize()
    assert np.array_equal(a1.cpu().numpy().T, r["actions"])
    assert torch.equal(a1, a2)
    assert torch.equal(tb.board, board0)                    # the agent only reads
    assert np.array_equal(tb.tcount.cpu().numpy(), r["c"].astype(np.int32) + 1)
    # stepping those actions gives the reference's next state
    tb.step(a1)
    b, h, d, k = _state(tb)
    assert np.array_equal(b, r["next_board"]) and np.array_equal(h.T, r["next_heads"])
    assert np.array_equal(d.T, r["next_dirs"]) and np.array_equal(k.T, r["next_deaths"])


@pytest.mark.parametrize("P", [2, 3, 4, 6])
def test_player_mask_leaves_other_rows(P):
    N, B = 19, 777
    tb = _tb(N, P, B)
    tb.rollout(7, seed=5)                                   # some trails, some dead players
    full = tb.sample_avoid(9, 0.3, advance=False)
    fill = torch.full((P, B), 77, dtype=torch.int8, device=tb.device)
    players = [p for p in range(P) if p % 2 == 1]
    out = tb.sample_avoid(9, 0.3, players=players, out=fill.clone(), advance=False)
    for p in range(P):
        want = full[p] if p in players else fill[p]
        assert torch.equal(out[p], want), p
    with pytest.raises(ValueError):
        tb.sample_avoid(players=[P])


def _check_rollout_against_loops(N, P, B, T, seed, noise, first_env_id=0, host=True):
    """rollout_avoid(T) == T x (sample_avoid; step(auto_reset)) on the device (state and stats) == the numpy + oracle loop."""
    fused, loop = _tb(N, P, B, first_env_id=first_env_id), _tb(N, P, B, first_env_id=first_env_id)
    fused.rollout_avoid(T, seed, noise)
    st = {k: torch.zeros_like(getattr(loop, k)) for k in STATS}
    for _ in range(T):
        loop.step(loop.sample_avoid(seed, noise), auto_reset=True)
    torch.cuda.synchronize()
    fs = _state(fused)
    for a, b in zip(fs, _state(loop)):
        assert np.array_equal(a, b)
    assert np.array_equal(fused.tcount.cpu().numpy(), loop.tcount.cpu().numpy())
    assert torch.equal(fused.results(), fused.results_from_columns())
    assert torch.equal(fused.results_packed(), fused.results_packed_from_columns())   # the 16-bit row the kernel packs, too
    assert fused.packed_rows_exact()
    if not host:
        return fused
    ref = tron_ref.HostLoop(N, P, B, fused.start_heads, fused.start_dirs)
    ref.run(T, seed, noise, first_env_id)
    for a, b in zip(fs, (ref.st.board, ref.st.heads, ref.st.dirs, ref.st.deaths)):
        assert np.array_equal(a, b)
    got = _stats(fused)
    for k in STATS:
        assert np.array_equal(got[k].view(getattr(ref.st, k).dtype), getattr(ref.st, k)), k
    return fused


@pytest.mark.parametrize("N", [15, 19, 20, 23, 40])
@pytest.mark.parametrize("P", [2, 3, 4])
def test_rollout_avoid_equals_loops(N, P):
    _check_rollout_against_loops(N, P, 333, 150, seed=1234 + N, noise=0.1, first_env_id=7)


@pytest.mark.parametrize("noise", [0.0, 1.0])
def test_rollout_avoid_noise_extremes(noise):
    _check_rollout_against_loops(19, 4, 200, 120, seed=3, noise=noise)


def test_rollout_avoid_six_players_fallback():
    _check_rollout_against_loops(20, 6, 300, 150, seed=99, noise=0.1)


@pytest.mark.parametrize("B", [1, 63, 65, 1000])
def test_rollout_avoid_ragged_batches(B):
    _check_rollout_against_loops(17, 4, B, 80, seed=B, noise=0.1)


def test_rollout_avoid_large_batch():
    B, N, P, T = 65536, 19, 4, 40
    fused = _check_rollout_against_loops(N, P, B, T, seed=2024, noise=0.1, host=False)
    assert int(fused.n_episodes.sum().item()) > 0


@pytest.mark.parametrize("P", [3, 4, 6])
def test_rollout_avoid_cross_launch(P):
    N, B = 20, 500
    one, two = _tb(N, P, B), _tb(N, P, B)
    one.rollout_avoid(130, 5, 0.1)
    two.rollout_avoid(47, 5, 0.1)
    two.rollout_avoid(83, 5, 0.1)
    torch.cuda.synchronize()
    for a, b in zip(_state(one), _state(two)):
        assert np.array_equal(a, b)
    for k, v in _stats(one).items():
        assert np.array_equal(v, _stats(two)[k]), k
    assert torch.equal(one.results(), two.results())


def test_avoid_episodes_are_longer_than_random():
    N, P, B, T = 19, 4, 4096, 200
    rnd, avo = _tb(N, P, B), _tb(N, P, B)
    rnd.rollout(T, 1)
    avo.rollout_avoid(T, 1, 0.1)
    mean = lambda tb: tb.len_sum.sum().item() / max(1, tb.n_episodes.sum().item())
    assert mean(avo) > 2 * mean(rnd)


class _HostSingle:
    """Host replay of TronSinglePlayerVectorEnv: learner = player 0, opponents on the avoid contract, done resets."""

    def __init__(self, N, P, B, sh, sd, seed, noise):
        self.loop = tron_ref.HostLoop(N, P, B, sh, sd)
        self.seed, self.noise = seed, noise

    def step(self, action):
        from oracle import oracle as O
        st = self.loop.st
        act = tron_ref.decide(st.N, st.board, st.heads, st.dirs, st.deaths, np.arange(st.B), st.tcount, self.seed, self.noise)
        st.tcount += 1
        act[0] = np.array([0, 1, -1], np.int8)[action]
        rew, term, _ = O.tron_step(st, act)
        done = (term != 0) | (st.deaths[0] != 0)
        self.loop.reset_games(done)
        return rew[0].copy(), done.astype(np.uint8), term.copy()


def test_single_player_vector_env_matches_host_replay():
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    N, P, B, K, seed, noise = 15, 4, 700, 60, 21, 0.1
    env = TronSinglePlayerVectorEnv(N, P, B, noise=noise, seed=seed, device="cuda:0")
    host = _HostSingle(N, P, B, env.batch.start_heads, env.batch.start_dirs, seed, noise)
    obs = env.reset()
    rng = np.random.default_rng(0)
    n_done = 0
    for _ in range(K):
        a = rng.integers(0, 3, size=B)
        obs, rew, done, info = env.step(torch.from_numpy(a).cuda())
        hr, hd, ht = host.step(a)
        assert np.array_equal(rew.cpu().numpy(), hr)
        assert np.array_equal(done.cpu().numpy(), hd)
        assert np.array_equal(info["terminal"].cpu().numpy(), ht)
        st = host.loop.st
        assert np.array_equal(obs["board"].reshape(B, -1).cpu().numpy(), st.board)
        assert np.array_equal(obs["heads"].cpu().numpy(), st.heads)
        assert np.array_equal(obs["directions"].cpu().numpy(), st.dirs)
        assert np.array_equal(obs["deaths"].cpu().numpy(), st.deaths)
        n_done += int(hd.sum())
    assert n_done > 0
    # player 0's relative observation is the state itself
    pl = torch.zeros((B,), dtype=torch.int8, device="cuda:0")
    o = env.batch.observe(pl)
    for k in ("board", "heads", "directions", "deaths"):
        assert torch.equal(o[k], obs[k])


def test_single_player_vector_env_graph_replay():
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    N, P, B, seed, noise = 19, 3, 512, 8, 0.1
    env = TronSinglePlayerVectorEnv(N, P, B, noise=noise, seed=seed, device="cuda:0")
    host = _HostSingle(N, P, B, env.batch.start_heads, env.batch.start_dirs, seed, noise)
    env.reset()
    action = torch.zeros((B,), dtype=torch.int64, device="cuda:0")
    rng = np.random.default_rng(1)
    # warm-up step on a side stream (as torch.cuda.graph wants), replayed on the host too
    a = rng.integers(0, 3, size=B)
    action.copy_(torch.from_numpy(a))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        env.step(action)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    host.step(a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # a chain of two kernels: no parallel branches
        obs, rew, done, info = env.step(action)
    for _ in range(25):
        a = rng.integers(0, 3, size=B)
        action.copy_(torch.from_numpy(a))
        g.replay()
        hr, hd, _ = host.step(a)
        torch.cuda.synchronize()
        assert np.array_equal(rew.cpu().numpy(), hr) and np.array_equal(done.cpu().numpy(), hd)
        assert np.array_equal(obs["board"].reshape(B, -1).cpu().numpy(), host.loop.st.board)
        assert np.array_equal(obs["heads"].cpu().numpy(), host.loop.st.heads)
