"""numpy restatement of crl_ttt_step_single / crl_blokus_step_single (include/colosseum_hip.h, "one learner against the
random agent") over the CPU oracle's own bindings: oracle.ttt_step / blokus_step / blokus_valid / blokus_observe and
philox4x32.  Written from the header's words, one game at a time; no code is shared with the kernels.

States are the oracle's TTTState / BlokusState (their ``tcount`` is the RNG step counter)."""
import numpy as np

from oracle import oracle as O

TAG_TTT = 0x54540000
TAG_BLOKUS = 0x424C0000
BLOKUS_TOP = 336000 + 1344000          # CRL_BLOKUS_EXT_BASE + CRL_BLOKUS_EXT_IDS
LIST_CAP = 8192


def _key(seed):
    return [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]


# ------------------------------------------------------------------ TicTacToe
def ttt_draw(seed, g, c, empty, n_cells):
    """crl_ttt_sample's action for step counter c of game g on a board whose empty cells are the mask `empty`."""
    n = bin(int(empty)).count("1")
    if n == 0:
        return -1
    w = int(O.philox4x32([g & 0xFFFFFFFF, (c >> 3) & 0xFFFFFFFF, 0, TAG_TTT], _key(seed))[(c >> 1) & 3])
    if c & 1:
        w = (w * (n + 1)) & 0xFFFFFFFF
    r = (w * n) >> 32
    cells = [i for i in range(n_cells) if (int(empty) >> i) & 1]
    return cells[r]


def _ttt_one(st, b):
    one = O.TTTState(st.dims, st.K, st.P, 1)
    one.occ[:, 0] = st.occ[:, b]
    one.winner[0], one.to_move[0] = st.winner[b], st.to_move[b]
    return one


def _ttt_empty(one):
    full = (1 << one.n_cells) - 1
    return full & ~int(np.bitwise_or.reduce(one.occ[:, 0]))


def ttt_step_single(st, seat, learner_action, seed, first_env_id=0, rel_mod=None, policy=None):
    """One call on every game of `st` (mutated, tcount included).  learner_action int64 [B] or None; `policy(b, one, c)`
    (instead of learner_action) returns the learner's int64 action from the state and step counter at its ply.
    Returns (reward int8, done uint8, winners int8, obs int8 [B, cells], valid uint32)."""
    P, B = st.P, st.B
    rel_mod = rel_mod or P
    reward = np.zeros(B, np.int8)
    done = np.zeros(B, np.uint8)
    winners = np.full(B, -1, np.int8)
    for b in range(B):
        s = int(seat[b]) % P
        one = _ttt_one(st, b)
        c = int(st.tcount[b])
        g = first_env_id + b
        learner = (learner_action is not None or policy is not None) and int(one.to_move[0]) == s
        opp = 0
        while learner or (int(one.to_move[0]) != s and opp < 2 * (P - 1)):
            if learner:
                v = int(policy(b, one, c)) if policy is not None else int(learner_action[b])
                act = v if -1 <= v < one.n_cells else -1
            else:
                act = ttt_draw(seed, g, c, _ttt_empty(one), one.n_cells)
                opp += 1
            learner = False
            c += 1
            _, term, ws = O.ttt_step(one, np.array([act], np.int8))
            if term[0]:
                done[b] = 1
                winners[b] = ws[0]
                reward[b] = 0 if ws[0] < 0 else (1 if ws[0] == s else -1)
                one.occ[:] = 0
                one.winner[0], one.to_move[0] = -1, 0
        st.occ[:, b] = one.occ[:, 0]
        st.winner[b], st.to_move[b] = one.winner[0], one.to_move[0]
        st.tcount[b] = c
    obs = st.board().astype(np.int16)
    rel = (np.asarray(seat, np.int64) % P)[:, None]
    obs = np.where(obs >= 0, (obs - rel) % rel_mod, -1).astype(np.int8)
    full = (1 << st.n_cells) - 1
    valid = (full & ~np.bitwise_or.reduce(st.occ, axis=0)).astype(np.uint32)
    return reward, done, winners, obs, valid


# ------------------------------------------------------------------ Blokus
def blokus_word(seed, g, c):
    return int(O.philox4x32([g & 0xFFFFFFFF, (c >> 2) & 0xFFFFFFFF, 0, TAG_BLOKUS], _key(seed))[c & 3])


def blokus_list(one, player=None):
    count, ids = O.blokus_valid(one, player=player, cap=LIST_CAP)
    assert count[0] <= LIST_CAP
    return ids[0, :count[0]]


def blokus_draw_rank(seed, g, c, n):
    return (blokus_word(seed, g, c) * n) >> 32


def _blk_one(st, b):
    one = O.BlokusState(1)
    for name in ("occ", "inv", "score", "round", "to_move"):
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
        one = _blk_one(st, b)
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
            c += 1
            if term[0]:
                done[b] = 1
                winners[b] = ws[0]
                reward[b] = blokus_rank_of(one.score[0], s)
                O.blokus_reset(one)
        for name in ("occ", "inv", "score", "round", "to_move"):
            getattr(st, name)[b] = getattr(one, name)[0]
        st.tcount[b] = c
    seat8 = (np.asarray(seat, np.int64) & 3).astype(np.int8)
    n_valid = O.blokus_valid(st, player=seat8)[0]
    ob, op, osc = O.blokus_observe(st, seat8)
    return reward, done, winners, n_valid, ob, op, osc
