"""What the GPU tests share: the device, tensors to numpy and back, and an oracle TicTacToe state as a TTTBatch."""
import numpy as np

DEV = "cuda:0"


def np_of(t):
    """a device tensor as a numpy array"""
    return t.cpu().numpy()


def u32_of(t):
    """an int32 device tensor as a uint32 numpy array (the bit masks)"""
    return np_of(t).view(np.uint32)


def to_dev(a):
    """a numpy array (copied: shared fixtures are read-only) as a device tensor, uint32 as the int32 of the same bits"""
    import torch
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def ttt_batch(st, first_env_id=0, tcount=None):
    """a TTTBatch holding the oracle state `st`, with its own step counters or `tcount`"""
    import torch
    from colosseumrl_amd.batched import TTTBatch
    tb = TTTBatch(st.dims, st.K, st.P, st.B, device=DEV, first_env_id=first_env_id)
    tb.occ.copy_(torch.from_numpy(st.occ.view(np.int32)))
    tb.winner.copy_(torch.from_numpy(st.winner))
    tb.to_move.copy_(torch.from_numpy(st.to_move))
    tb.tcount.copy_(torch.from_numpy((st.tcount if tcount is None else tcount).view(np.int32)))
    return tb


def same_ttt_state(tb, st):
    """the TTTBatch holds the oracle state `st`, step counters included"""
    assert np.array_equal(u32_of(tb.occ), st.occ)
    assert np.array_equal(np_of(tb.winner), st.winner) and np.array_equal(np_of(tb.to_move), st.to_move)
    assert np.array_equal(u32_of(tb.tcount), st.tcount)


TRON_STATS = ("tcount", "tstep", "n_episodes", "win_count", "len_sum", "ret_sum", "last_winners", "last_len")


def tron_put(tb, board, heads, dirs, deaths):
    """load a position (numpy arrays shaped as the batch's) into a TronBatch"""
    import torch
    for t, a in zip((tb.board, tb.heads, tb.dirs, tb.deaths), (board, heads, dirs, deaths)):
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def tron_state(tb):
    """[board, heads, dirs, deaths] of a TronBatch as numpy arrays"""
    return [np_of(t) for t in (tb.board, tb.heads, tb.dirs, tb.deaths)]


def tron_stats(tb):
    """the counters and rollout statistics of a TronBatch as numpy arrays, by name"""
    return {k: np_of(getattr(tb, k)) for k in TRON_STATS}


def blokus_batch(st, first_env_id=0, tcount=None):
    """a BlokusBatch holding the oracle state `st`, with its own step counters or `tcount`"""
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    bb = BlokusBatch(st.B, device=DEV, first_env_id=first_env_id)
    for name in ("occ", "inv", "score", "round", "to_move"):
        getattr(bb, name).copy_(torch.from_numpy(getattr(st, name).view(np.int32)))
    bb.tcount.copy_(torch.from_numpy((st.tcount if tcount is None else tcount).view(np.int32)))
    return bb


def first_episodes(env, policy, max_steps):
    """Every game's first episode in a single-player vector env that was just reset: steps it with policy(env, t), t = 0, 1,
    ... for at most max_steps steps (it stops at a multiple of 20 steps once every game has been done), and requires that
    every game was done by then.  -> device tensors [B]: the reward at the game's first `done`, the rewards summed (int64)
    and the steps counted while its first episode ran."""
    import torch
    B = env.num_envs
    live = torch.ones(B, dtype=torch.bool, device=DEV)
    last, ret, steps = None, torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    for t in range(max_steps):
        _, reward, done, _ = env.step(policy(env, t))
        last = torch.zeros_like(reward) if last is None else last
        ret += torch.where(live, reward.to(torch.int64), 0)
        steps += live.to(torch.int64)
        last = torch.where(live & (done != 0), reward, last)
        live &= done == 0
        if t % 20 == 19 and not bool(live.any()):
            break
    assert not bool(live.any())
    return last, ret, steps


def tron_device_evaluator(leaves):
    """an integer evaluator of the Tron tree searches' pending leaves in torch operations on the device (a hash of the
    observed board and the seat's head): (prior int16 [B, 3], value int32 [B]) for TronBatch.puct_backup"""
    import torch
    b = leaves["obs_board"].to(torch.int32)
    wgt = torch.arange(1, b.shape[1] + 1, device=b.device, dtype=torch.int32)
    h = ((b + 2) * (wgt % 251)).sum(dim=1, keepdim=True) + leaves["obs_heads"][0].to(torch.int32).view(-1, 1) * 977
    prior = ((h * 31 + torch.arange(1, 4, device=b.device, dtype=torch.int32) * 7919) % 32749).to(torch.int16)
    value = ((h.view(-1) * 131) % 65537).to(torch.int32)
    return prior, value
