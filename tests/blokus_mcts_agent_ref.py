"""Plain-Python restatement of the Blokus search agent ("the tree search as a seated agent of Blokus" in
include/colosseum_hip.h): crl_blokus_sample_mcts, crl_blokus_rollout_mcts and crl_blokus_step_single_mcts over the CPU
oracle's bindings, the search itself tests/blokus_mcts_ref.search, the draws rng_ref.philox's.  Written from the header's
words, one game and one ply at a time; no code is shared with the kernel.

States are the oracle's BlokusState (``tcount`` is the step counter); the three calls mutate theirs as the C entries do.
``log``, where given, is a list that grows by one (b, c, kind) per agent ply, kind in "pass", "noisy", "searched", and by
(b, c, "learner") / (b, c, "restart") in step_single_mcts, in the order they happen in game b."""
import math

import numpy as np

from oracle import oracle as O
from tests import blokus_mcts_ref as M
from tests import rng_ref as RNG
from tests.blokus_ref import BLOKUS_TOP, M32, _FIELDS, blokus_draw_rank, blokus_list, blokus_one, blokus_rank_of

NOISE_BITS = 0xC0000000                    # both top bits of the second counter word: no playout, widening or entry block


def threshold(noise):
    """thr = min(2^32, ceil(noise * 2^32))"""
    assert 0.0 <= noise <= 1.0
    return min(2 ** 32, math.ceil(noise * 4294967296.0))


def noise_word(seed, g, c):
    """u of rule 2: the word that decides whether the ply at step counter c of game g is noisy"""
    return int(RNG.philox(g, NOISE_BITS | (c >> 2), 0, M.TAG, seed)[c & 3])


def agent_action(one, c, g, seed, W, S, R, cexp, noise, kinds=None):
    """the agent's move on the one-game state `one` (not written) at step counter c of game g; kinds: a list that gets
    what the ply was"""
    note = kinds.append if kinds is not None else (lambda kind: None)
    ids = blokus_list(one)
    n = len(ids)
    if n == 0:
        note("pass")
        return -1
    if noise_word(seed, g, c) < threshold(noise):
        note("noisy")
        return int(ids[blokus_draw_rank(seed, g, c, n)])
    note("searched")
    return int(M.search(one, S, R, W, cexp, seed, g, c)[4])


def _agent(one, b, c, g, seed, search, log):
    kinds = []
    act = agent_action(one, c, g, seed, *search, kinds=kinds)
    if log is not None:
        log.append((b, c, kinds[0]))
    return act


def sample_mcts(st, seed, W, S, R, cexp, noise, first_env_id=0, advance=True, log=None):
    """crl_blokus_sample_mcts -> action int32 [B]"""
    act = np.zeros(st.B, np.int32)
    for b in range(st.B):
        c = int(st.tcount[b])
        act[b] = _agent(blokus_one(st, b), b, c, (first_env_id + b) & M32, seed, (W, S, R, cexp, noise), log)
        if advance:
            st.tcount[b] = (c + 1) & M32
    return act


def rollout_mcts(st, T, seed, W, S, R, cexp, noise, first_env_id=0, log=None, games=None):
    """crl_blokus_rollout_mcts on the games `games` (default: all) of `st`: state, counters and statistics"""
    for b in (range(st.B) if games is None else games):
        one, g = blokus_one(st, b), (first_env_id + b) & M32
        c, ts = int(st.tcount[b]), int(st.tstep[b])
        for _ in range(T):
            act = _agent(one, b, c, g, seed, (W, S, R, cexp, noise), log)
            r, term, ws = O.blokus_step(one, np.array([act], np.int32))
            assert r[0] >= 0 or term[0], "the agent's action raised"
            c, ts = (c + 1) & M32, ts + 1
            if term[0]:
                st.n_episodes[b] += 1
                st.len_sum[b] += ts
                for q in range(4):
                    st.win_count[q, b] += (int(ws[0]) >> q) & 1
                    st.score_sum[q, b] += one.score[0, q]
                O.blokus_reset(one)
                ts = 0
        for name in _FIELDS:
            getattr(st, name)[b] = getattr(one, name)[0]
        st.tcount[b], st.tstep[b] = c, ts


def step_single_mcts(st, seat, learner_action, seed, W, S, R, cexp, noise, first_env_id=0, rank=False, log=None):
    """crl_blokus_step_single_mcts: crl_blokus_step_single's steps 1 to 5 with the search agent in step 2.  learner_action
    int64 [B] or None.  -> (reward int8, done uint8, winners uint8, n_valid int32, obs_board, obs_pieces, obs_score)"""
    B = st.B
    reward, done, winners = np.zeros(B, np.int8), np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    for b in range(B):
        s = int(seat[b]) & 3
        one, g, c = blokus_one(st, b), (first_env_id + b) & M32, int(st.tcount[b])
        learner = learner_action is not None and (int(one.to_move[0]) & 3) == s
        opp = 0
        while learner or ((int(one.to_move[0]) & 3) != s and opp < 6):
            if learner:
                v = int(learner_action[b])
                if rank:
                    ids = blokus_list(one)
                    act = int(ids[v]) if 0 <= v < len(ids) else -1
                else:
                    act = -1 if v < 0 else min(v, BLOKUS_TOP)
                if log is not None:
                    log.append((b, c, "learner"))
            else:
                act = _agent(one, b, c, g, seed, (W, S, R, cexp, noise), log)
                opp += 1
            was_learner, learner = learner, False
            r, term, ws = O.blokus_step(one, np.array([act], np.int32))
            if r[0] < 0 and not term[0]:       # the reference raises: the game stays as it was, nobody else plays
                assert was_learner, "the agent's action raised"
                reward[b] = r[0]
                break
            c = (c + 1) & M32
            if term[0]:
                done[b], winners[b], reward[b] = 1, ws[0], blokus_rank_of(one.score[0], s)
                O.blokus_reset(one)
                if log is not None:
                    log.append((b, c, "restart"))
        for name in _FIELDS:
            getattr(st, name)[b] = getattr(one, name)[0]
        st.tcount[b] = c
    seat8 = (np.asarray(seat, np.int64) & 3).astype(np.int8)
    n_valid = O.blokus_valid(st, player=seat8)[0]
    ob, op, osc = O.blokus_observe(st, seat8)
    return reward, done, winners, n_valid, ob, op, osc
