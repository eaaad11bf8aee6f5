"""One learner against the random agent (crl_ttt_step_single / crl_blokus_step_single) on the host: the numpy
restatement of the header's contract (tests/ttt_ref.py, tests/blokus_ref.py) against the oracle's rollouts -- a learner that
plays the random agent's own draw at its own step counter must leave every game exactly where the rollout of that game leaves it
after as many plies --, and the argument checks of the two C entry points (they fail before any device work)."""
import ctypes as C

import numpy as np
import pytest

from tests import blokus_ref as R
from tests import ttt_ref
from tests import ttt_probes as TP
from tests.host_util import D, lib as _lib, ttt_context

TTT_CONFIGS = TP.INSTANCE_ROWS              # the rows tests/test_gpu_single_turn.py runs


def _ttt_learner_is_agent(seed):
    def policy(st):
        return ttt_ref.sample(st, seed, ttt_ref.random_agent, advance=False).astype(np.int64)
    return policy


@pytest.mark.parametrize("dims,K,P", TTT_CONFIGS, ids=TP.INSTANCE_IDS)
def test_ttt_learner_as_agent_is_the_rollout(dims, K, P):
    from oracle import oracle as O
    B, seed, calls = 3 * P, 0x5EED + P, 14
    seat = np.array([b % P for b in range(B)], np.int8)               # every seat
    st = O.TTTState(dims, K, P, B)
    ttt_ref.step_single(st, seat, None, seed, ttt_ref.random_agent)                            # reset(): on to the learner's turn
    assert all(int(st.to_move[b]) == seat[b] for b in range(B))
    n_done = 0
    for _ in range(calls):
        _, done, _, _, _ = ttt_ref.step_single(st, seat, None, seed, ttt_ref.random_agent, policy=_ttt_learner_is_agent(seed))
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
    ttt_ref.step_single(st, seat, None, seed, ttt_ref.random_agent)
    before = st.occ.copy()
    tc = st.tcount.copy()
    # a pass, an out-of-range value and an occupied cell leave the learner's marks alone and still cost one draw each
    occupied = int(np.flatnonzero(st.board()[1] >= 0)[0])
    act = np.array([-1, occupied, 9, -7, 2 ** 40, -1], np.int64)
    reward, done, winners, obs, valid = ttt_ref.step_single(st, seat, act, seed, ttt_ref.random_agent)
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
    legal = R.blokus_list(R.blokus_one(st, 0))
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
def test_abi_revision():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _native.lib().crl_version() == 113
    assert _native.CRL_STEP_RANK_ACTION == 8


def test_ttt_step_single_argument_checks():
    lib = _lib()
    with ttt_context() as h:
        def call(ptrs=(D,) * 11, rel_mod=2, flags=0, B=4, ctx=h):
            return lib.crl_ttt_step_single(ctx, B, 1, 0, *ptrs, rel_mod, flags, None)
        for i in range(11):
            if i == 4:                    # learner_action: NULL is the "advance to the learner's turn" call
                continue
            ptrs = [D] * 11
            ptrs[i] = None
            assert call(ptrs=tuple(ptrs)) == -1 and b"NULL" in lib.crl_last_error()
        assert call(rel_mod=0) == -1 and b"rel_mod" in lib.crl_last_error()
        for flags in (1, 8, 0x80000000):
            assert call(flags=flags) == -1 and b"flags" in lib.crl_last_error()
        assert call(B=0) == -1
        assert call(ctx=None) == -1 and b"tictactoe" in lib.crl_last_error()
        unaligned = [D] * 11
        unaligned[9] = C.c_void_p(65)
        assert call(ptrs=tuple(unaligned)) == -1 and b"aligned" in lib.crl_last_error()
    with ttt_context(1, 1, 2, 2, 3) as small:  # a board with fewer cells than players: a fresh game could end before the learner
        assert lib.crl_ttt_step_single(small, 4, 1, 0, *([D] * 11), 3, 0, None) == -1
        assert b"cells" in lib.crl_last_error()


def test_blokus_step_single_argument_checks():
    lib = _lib()
    with ttt_context() as tt:
        def call(ptrs=(D,) * 15, flags=0, ctx=None, B=4):
            return lib.crl_blokus_step_single(ctx, B, 1, 0, *ptrs, flags, None)
        for i in range(15):
            if i == 6:                    # learner_action may be NULL
                continue
            ptrs = [D] * 15
            ptrs[i] = None
            assert call(ptrs=tuple(ptrs)) == -1 and b"NULL" in lib.crl_last_error()
        for flags in (1, 2, 4, 16, 0x80000000):
            assert call(flags=flags) == -1 and b"flags" in lib.crl_last_error()
        unaligned = [D] * 15
        unaligned[12] = C.c_void_p(66)
        assert call(ptrs=tuple(unaligned)) == -1 and b"aligned" in lib.crl_last_error()
        # every argument right but the context: no context, or one of another game
        assert call() == -1 and b"blokus context" in lib.crl_last_error()
        assert call(flags=8) == -1 and b"blokus context" in lib.crl_last_error()
        assert call(ctx=tt) == -1 and b"blokus context" in lib.crl_last_error()
