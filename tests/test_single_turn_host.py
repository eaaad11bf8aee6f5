"""One learner against the random agent (crl_ttt_step_single / crl_blokus_step_single) on the host: the numpy
restatement of the header's contract (tests/single_ref.py) against the oracle's rollouts -- a learner that plays the
random agent's own draw at its own step counter must leave every game exactly where the rollout of that game leaves it
after as many plies --, and the argument checks of the two C entry points (they fail before any device work)."""
import ctypes as C

import numpy as np
import pytest

from tests import single_ref as R
from tests import ttt_probes as TP

TTT_CONFIGS = TP.INSTANCE_ROWS              # the rows tests/test_gpu_single_turn.py runs


def _ttt_learner_is_agent(seed):
    def policy(b, one, c):
        return R.ttt_draw(seed, b, c, R._ttt_empty(one), one.n_cells)
    return policy


@pytest.mark.parametrize("dims,K,P", TTT_CONFIGS, ids=TP.INSTANCE_IDS)
def test_ttt_learner_as_agent_is_the_rollout(dims, K, P):
    from oracle import oracle as O
    B, seed, calls = 3 * P, 0x5EED + P, 14
    seat = np.array([b % P for b in range(B)], np.int8)               # every seat
    st = O.TTTState(dims, K, P, B)
    R.ttt_step_single(st, seat, None, seed)                            # reset(): on to the learner's turn
    assert all(int(st.to_move[b]) == seat[b] for b in range(B))
    n_done = 0
    for _ in range(calls):
        _, done, _, _, _ = R.ttt_step_single(st, seat, None, seed, policy=_ttt_learner_is_agent(seed))
        n_done += int(done.sum())
        assert all(int(st.to_move[b]) == seat[b] for b in range(B))
    assert n_done > 0                                                  # the comparison runs across restarts
    for g in range(B):
        ref = O.TTTState(dims, K, P, 1)
        O.ttt_rollout(ref, seed, g, int(st.tcount[g]))
        assert np.array_equal(ref.occ[:, 0], st.occ[:, g]), g
        assert ref.winner[0] == st.winner[g] and ref.to_move[0] == st.to_move[g], g


def test_ttt_outcomes_and_passes():
    from oracle import oracle as O
    P, B, seed = 2, 6, 9
    st = O.TTTState((3, 3), 3, P, B)
    seat = np.array([0, 1, 0, 1, 0, 1], np.int8)
    R.ttt_step_single(st, seat, None, seed)
    before = st.occ.copy()
    tc = st.tcount.copy()
    # a pass, an out-of-range value and an occupied cell leave the learner's marks alone and still cost one draw each
    occupied = int(np.flatnonzero(st.board()[1] >= 0)[0])
    act = np.array([-1, occupied, 9, -7, 2 ** 40, -1], np.int64)
    reward, done, winners, obs, valid = R.ttt_step_single(st, seat, act, seed)
    for b in range(B):
        s = int(seat[b])
        assert st.occ[s, b] == before[s, b]
        assert st.tcount[b] == tc[b] + P                               # one learner ply + P - 1 opponent plies
    assert (done == 0).all() and (reward == 0).all() and (winners == -1).all()
    # the observation is relative to the learner: its own marks are 0
    for b in range(B):
        bd = st.board()[b]
        assert np.array_equal(obs[b] == 0, bd == seat[b]) and np.array_equal(obs[b] < 0, bd < 0)


@pytest.mark.parametrize("rank", [False, True], ids=["id", "rank"])
def test_blokus_learner_as_agent_is_the_rollout(rank):
    from oracle import oracle as O
    B, seed, calls = 4, 77, 22
    seat = np.array([0, 1, 2, 3], np.int8)
    st = O.BlokusState(B)
    R.blokus_step_single(st, seat, None, seed)
    assert list(st.to_move) == [0, 1, 2, 3]

    def policy(b, one, c, ids):
        r = R.blokus_draw_rank(seed, b, c, len(ids))
        if rank:
            return r if len(ids) else -1
        return int(ids[r]) if len(ids) else -1
    for _ in range(calls):
        reward, done, winners, n_valid, _, _, _ = R.blokus_step_single(st, seat, None, seed, rank=rank, policy=policy)
        assert (reward >= 0).all() and (reward <= 3).all()
        assert list(st.to_move) == [0, 1, 2, 3]
    for g in range(B):
        ref = O.BlokusState(1)
        O.blokus_rollout(ref, seed, g, int(st.tcount[g]))
        for name in ("occ", "inv", "score", "round", "to_move"):
            assert np.array_equal(getattr(ref, name)[0], getattr(st, name)[g]), (g, name)


def test_blokus_error_codes_leave_the_game():
    from oracle import oracle as O
    B, seed = 5, 3
    seat = np.zeros(B, np.int8)
    st = O.BlokusState(B)
    R.blokus_step_single(st, seat, None, seed)
    legal = R.blokus_list(R._blk_one(st, 0))
    # monomino with shift 1 names no cell of the piece: IndexError; ids past the last extended id: BAD_ACTION;
    # a legal id plays; -5 is a pass
    act = np.array([O.blokus_encode(0, 0, 0, 0, 1), R.BLOKUS_TOP, 2 ** 40, int(legal[0]), -5], np.int64)
    snap = {n: getattr(st, n).copy() for n in ("occ", "inv", "score", "round", "to_move", "tcount")}
    reward, done, winners, n_valid, _, _, _ = R.blokus_step_single(st, seat, act, seed)
    assert list(reward) == [-1, -3, -3, 0, 0] and (done == 0).all()
    for b in range(3):
        for n, v in snap.items():
            assert np.array_equal(getattr(st, n)[b], v[b]), (b, n)
    assert st.tcount[3] == snap["tcount"][3] + 4 and st.tcount[4] == snap["tcount"][4] + 4
    assert not (st.inv[3, 0] >> (int(legal[0]) // 16000)) & 1
    # ValueError: the piece just played is no longer held (the learner's next turn, the same id again)
    act2 = np.full(B, -1, np.int64)
    act2[3] = int(legal[0])
    reward, _, _, _, _, _, _ = R.blokus_step_single(st, seat, act2, seed)
    assert reward[3] == -2


# ---- argument checks of the C entry points (rejected before anything touches a device)
def _lib():
    from colosseumrl_amd import _native
    return _native.lib()


def test_abi_revision():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _native.lib().crl_version() == 113
    assert _native.CRL_STEP_RANK_ACTION == 8


def test_ttt_step_single_argument_checks():
    lib = _lib()
    h = C.c_void_p()
    assert lib.crl_ttt_create(1, 3, 3, 3, 2, C.byref(h)) == 0
    d = C.c_void_p(64)                    # never dereferenced: every call below is rejected by its checks
    try:
        def call(ptrs=(d,) * 11, rel_mod=2, flags=0, B=4, ctx=h):
            return lib.crl_ttt_step_single(ctx, B, 1, 0, *ptrs, rel_mod, flags, None)
        for i in range(11):
            if i == 4:                    # learner_action: NULL is the "advance to the learner's turn" call
                continue
            ptrs = [d] * 11
            ptrs[i] = None
            assert call(ptrs=tuple(ptrs)) == -1 and b"NULL" in lib.crl_last_error()
        assert call(rel_mod=0) == -1 and b"rel_mod" in lib.crl_last_error()
        for flags in (1, 8, 0x80000000):
            assert call(flags=flags) == -1 and b"flags" in lib.crl_last_error()
        assert call(B=0) == -1
        assert call(ctx=None) == -1 and b"tictactoe" in lib.crl_last_error()
        unaligned = [d] * 11
        unaligned[9] = C.c_void_p(65)
        assert call(ptrs=tuple(unaligned)) == -1 and b"aligned" in lib.crl_last_error()
    finally:
        lib.crl_destroy(h)
    small = C.c_void_p()                  # a board with fewer cells than players: a fresh game could end before the learner
    assert lib.crl_ttt_create(1, 1, 2, 2, 3, C.byref(small)) == 0
    try:
        assert lib.crl_ttt_step_single(small, 4, 1, 0, *([d] * 11), 3, 0, None) == -1
        assert b"cells" in lib.crl_last_error()
    finally:
        lib.crl_destroy(small)


def test_blokus_step_single_argument_checks():
    lib = _lib()
    d = C.c_void_p(64)
    tt = C.c_void_p()
    assert lib.crl_ttt_create(1, 3, 3, 3, 2, C.byref(tt)) == 0
    try:
        def call(ptrs=(d,) * 15, flags=0, ctx=None, B=4):
            return lib.crl_blokus_step_single(ctx, B, 1, 0, *ptrs, flags, None)
        for i in range(15):
            if i == 6:                    # learner_action may be NULL
                continue
            ptrs = [d] * 15
            ptrs[i] = None
            assert call(ptrs=tuple(ptrs)) == -1 and b"NULL" in lib.crl_last_error()
        for flags in (1, 2, 4, 16, 0x80000000):
            assert call(flags=flags) == -1 and b"flags" in lib.crl_last_error()
        unaligned = [d] * 15
        unaligned[12] = C.c_void_p(66)
        assert call(ptrs=tuple(unaligned)) == -1 and b"aligned" in lib.crl_last_error()
        # every argument right but the context: no context, or one of another game
        assert call() == -1 and b"blokus context" in lib.crl_last_error()
        assert call(flags=8) == -1 and b"blokus context" in lib.crl_last_error()
        assert call(ctx=tt) == -1 and b"blokus context" in lib.crl_last_error()
    finally:
        lib.crl_destroy(tt)
