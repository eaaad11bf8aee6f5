"""numpy restatement of crl_blokus_step_single ("one learner against the random agent") and crl_blokus_playout ("batched
random playouts") of include/colosseum_hip.h over the CPU oracle's own bindings: oracle.blokus_step / blokus_valid /
blokus_observe, the draws from rng_ref.philox.  Written from the header's words, one game and one playout at a time; no
code is shared with the kernels.

States are the oracle's BlokusState (``tcount`` is the RNG step counter).  blokus_playout never writes its state;
``tcount`` (uint32 [B] or None = 0) is its counter base, and it returns numpy arrays shaped as the C outputs: wins uint32
[B, A, 4], played / len_sum uint32 [B, A], score_sum int32 [B, A, 4]."""
import numpy as np

from oracle import oracle as O
from tests import rng_ref as RNG

BLOKUS_TOP = 336000 + 1344000          # CRL_BLOKUS_EXT_BASE + CRL_BLOKUS_EXT_IDS
LIST_CAP = 8192
M32 = RNG.M32
_FIELDS = ("occ", "inv", "score", "round", "to_move")


def blokus_word(seed, g, c, c2=0, tag=RNG.CRL_TAG_BLOKUS):
    """the Philox word of step counter c of game g: block c >> 2, word c & 3 (c2: (a << 16) | r of a playout row)"""
    return int(RNG.philox(g, c >> 2, c2, tag, seed)[c & 3])


def blokus_draw_rank(seed, g, c, n):
    return (blokus_word(seed, g, c) * n) >> 32


def blokus_list(one, player=None):
    """the legal dense ids of the mover (or of `player`) in reference order"""
    count, ids = O.blokus_valid(one, player=player, cap=LIST_CAP)
    assert count[0] <= LIST_CAP
    return ids[0, :count[0]]


def blokus_one(st, b):
    """a one-game oracle state holding game b of `st`"""
    one = O.BlokusState(1)
    for name in _FIELDS:
        getattr(one, name)[0] = getattr(st, name)[b]
    return one


def blokus_rank_of(score, s):
    """crl_blokus_step's reward rule with the mover replaced by s"""
    return sum(1 for c in range(4) if score[c] < score[s] or (score[c] == score[s] and c < s))


def blokus_step_single(st, seat, learner_action, seed, first_env_id=0, rank=False, policy=None):
    """One call on every game of `st` (mutated).  learner_action int64 [B] or None; `policy(b, one, c, ids)` returns the
    learner's int64 action (ids: its ordered legal list).  Returns (reward int8, done uint8, winners uint8, n_valid int32,
    obs_board, obs_pieces, obs_score)."""
    B = st.B
    reward = np.zeros(B, np.int8)
    done = np.zeros(B, np.uint8)
    winners = np.zeros(B, np.uint8)
    for b in range(B):
        s = int(seat[b]) & 3
        one = blokus_one(st, b)
        c = int(st.tcount[b])
        g = first_env_id + b
        learner = (learner_action is not None or policy is not None) and (int(one.to_move[0]) & 3) == s
        opp = 0
        while learner or ((int(one.to_move[0]) & 3) != s and opp < 6):
            if learner:
                ids = blokus_list(one) if (rank or policy is not None) else None
                v = int(policy(b, one, c, ids)) if policy is not None else int(learner_action[b])
                if rank:
                    act = int(ids[v]) if 0 <= v < len(ids) else -1
                else:
                    act = -1 if v < 0 else min(v, BLOKUS_TOP)
            else:
                ids = blokus_list(one)
                act = int(ids[blokus_draw_rank(seed, g, c, len(ids))]) if len(ids) else -1
                opp += 1
            was_learner, learner = learner, False
            r, term, ws = O.blokus_step(one, np.array([act], np.int32))
            if r[0] < 0 and not term[0]:
                assert was_learner, "a drawn action raised"
                reward[b] = r[0]
                break
            c = (c + 1) & M32
            if term[0]:
                done[b] = 1
                winners[b] = ws[0]
                reward[b] = blokus_rank_of(one.score[0], s)
                O.blokus_reset(one)
        for name in _FIELDS:
            getattr(st, name)[b] = getattr(one, name)[0]
        st.tcount[b] = c
    seat8 = (np.asarray(seat, np.int64) & 3).astype(np.int8)
    n_valid = O.blokus_valid(st, player=seat8)[0]
    ob, op, osc = O.blokus_observe(st, seat8)
    return reward, done, winners, n_valid, ob, op, osc


def blokus_random_plies(one, seed, g, c, c2=0, tag=RNG.CRL_TAG_BLOKUS_PLAYOUT, max_plies=None):
    """The playout's ply loop on the one-game state `one` (mutated, never reset): random plies from step counter c up to
    the first terminal one, or `max_plies` of them.  -> (winners mask or None while the game goes on, plies played, the
    counter after them).  With tag=CRL_TAG_BLOKUS and c2=0 the draws are the rollout's."""
    plies = 0
    while max_plies is None or plies < max_plies:
        ids = blokus_list(one)
        word = blokus_word(seed, g, c, c2, tag)
        act = int(ids[(word * len(ids)) >> 32]) if len(ids) else -1
        _, term, ws = O.blokus_step(one, np.array([act], np.int32))
        plies += 1
        c = (c + 1) & M32
        if term[0]:
            return int(ws[0]), plies, c
    return None, plies, c


def blokus_one_playout(st, b, seed, g, c0, first, a, r, tag=RNG.CRL_TAG_BLOKUS_PLAYOUT):
    """(winners mask, plies, final scores) of playout r of row (b, a); `first` the candidate id or None"""
    one = blokus_one(st, b)
    if first is not None:
        _, term, ws = O.blokus_step(one, np.array([first], np.int32))
        if term[0]:
            return int(ws[0]), 1, one.score[0].copy()
    mask, plies, _ = blokus_random_plies(one, seed, g, c0, (a << 16) | r, tag)
    return mask, plies + (first is not None), one.score[0].copy()


def blokus_playout(st, seed, R, cand=None, A=1, first_env_id=0, tcount=None, rows=None):
    """crl_blokus_playout on the oracle state `st`.  rows: optional iterable of (b, a) to compute (the others stay 0)."""
    B = st.B
    if cand is None:
        assert A == 1
    else:
        cand = np.asarray(cand, np.int64)
        assert cand.shape == (B, A)
    wins = np.zeros((B, A, 4), np.uint32)
    played = np.zeros((B, A), np.uint32)
    len_sum = np.zeros((B, A), np.uint32)
    score_sum = np.zeros((B, A, 4), np.int32)
    todo = {}
    for b, a in (rows if rows is not None else [(b, a) for b in range(B) for a in range(A)]):
        todo.setdefault(int(b), []).append(int(a))
    for b, columns in todo.items():
        legal = set(int(i) for i in blokus_list(blokus_one(st, b))) if cand is not None else None
        c0 = 0 if tcount is None else int(tcount[b])
        for a in columns:
            first = None
            if cand is not None:
                v = int(cand[b, a])
                if v not in legal:
                    continue                                 # not a legal dense id of the mover: the row is skipped
                first = v
            for r in range(R):
                mask, plies, score = blokus_one_playout(st, b, seed, first_env_id + b, c0, first, a, r)
                for p in range(4):
                    wins[b, a, p] += (mask >> p) & 1
                len_sum[b, a] += plies
                score_sum[b, a] += score
            played[b, a] = R
    return wins, played, len_sum, score_sum
