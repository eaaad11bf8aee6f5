"""The Blokus tree search with progressive widening (crl_blokus_mcts) on the GPU: bit-exact against the plain-Python
restatement (tests/blokus_mcts_ref.py) on six positions with both mappings (R = 1: a wave per tree, R = 5: a workgroup per
tree) and both kinds of root, and the properties that need no restatement on a larger batch."""
import functools
import math

import numpy as np
import pytest

from tests import blokus_mcts_ref as M
from tests import blokus_positions as BP
from tests.blokus_ref import blokus_list, blokus_one
from tests.gpu_util import DEV, blokus_batch, np_of, to_dev, u32_of

pytestmark = pytest.mark.gpu

SEED, FIRST_ENV_ID, S, W = 0x5EA7C4, 4000, 24, 4
NAMES = ["empty", "plies12", "plies40", "must_pass", "finished", "tcount_wrap"]
KEYS = ("ids", "visits", "value", "nodes", "best")


@functools.lru_cache(maxsize=None)
def _positions():
    """(state of six positions, tcount): the empty board; a game after 12 and one after 40 random plies; one whose mover
    must pass while another player can move; a finished game; a small position at tcount = 2^32 - 2"""
    from oracle import oracle as O
    empty, p12, p40 = O.BlokusState(1), O.BlokusState(1), O.BlokusState(1)
    O.blokus_rollout(p12, 41, 500, 12)
    O.blokus_rollout(p40, 42, 501, 40)
    assert not p12.n_episodes.any() and not p40.n_episodes.any()
    late = BP.late(24)
    must_pass = BP.clone(late, [int(np.flatnonzero(BP.late_kinds(late)[0] >= 1)[0])])
    tiny = BP.tiny_inventories(12)
    n_legal = BP.counts(tiny)[np.arange(tiny.B), tiny.to_move & 3]
    wrap = BP.clone(tiny, [int(np.flatnonzero(n_legal >= 6)[0])])
    st = BP.concat([empty, p12, p40, must_pass, BP.finished(1), wrap])
    legal = [len(blokus_list(blokus_one(st, b))) for b in range(st.B)]
    assert legal[0] > 0 and legal[1] > 0 and legal[2] > 0 and legal[3] == 0 and legal[4] == 0 and legal[5] >= 6
    assert BP.counts(st)[3].sum() > 0 and BP.counts(st)[4].sum() == 0
    return st, np.array([0, 5, 13, 9, 3, 2 ** 32 - 2], np.uint32)


@functools.lru_cache(maxsize=None)
def _candidates():
    """int32 [6, 5]: a legal id, a dense id that is not legal, another legal id, the first one again, -1 (a mover without
    legal actions gets no playable column: the row is skipped)"""
    st, _ = _positions()
    cand = np.full((st.B, 5), -1, np.int32)
    for b in range(st.B):
        legal = [int(i) for i in blokus_list(blokus_one(st, b))]
        illegal = next(i for i in range(1000, 336000) if i not in set(legal))
        first = legal[len(legal) // 2] if legal else illegal
        cand[b] = [first, illegal, legal[0] if legal else 336000, first, -1]
    return cand


def _run(bb, *args, **kw):
    o = bb.mcts(*args, **kw)
    return {k: np_of(o[k]).copy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def _gpu(Rn, with_cand):
    st, tcount = _positions()
    bb = blokus_batch(st, FIRST_ENV_ID, tcount)
    return _run(bb, S, Rn, to_dev(_candidates()) if with_cand else None, W, SEED, 1.0)


@pytest.mark.parametrize("with_cand", [False, True], ids=["widening_root", "candidate_root"])
@pytest.mark.parametrize("Rn", [1, 5])
@pytest.mark.parametrize("b", range(6), ids=NAMES)
def test_bit_exact(b, Rn, with_cand):
    st, tcount = _positions()
    got = _gpu(Rn, with_cand)
    want = M.search(blokus_one(st, b), S, Rn, W, 256, SEED, FIRST_ENV_ID + b, int(tcount[b]),
                    [int(x) for x in _candidates()[b]] if with_cand else None)
    have = tuple(got[k][b].tolist() for k in KEYS)
    print(have, want)
    assert have == (want[0], want[1], want[2], want[3], want[4])
    if with_cand and b in (3, 4):
        assert want[3] == 0 and want[4] == -2                   # no playable column: skipped
    if not with_cand and b in (3, 4):
        assert want[0] == [-1, -2, -2, -2] and want[1][0] == S  # the pass is the only child


def test_one_simulation():
    st, tcount = _positions()
    bb = blokus_batch(st, FIRST_ENV_ID, tcount)
    for Rn in (1, 5):
        o = _run(bb, 1, Rn, None, W, SEED)
        assert (o["visits"][:, 0] == 1).all() and not o["visits"][:, 1:].any() and (o["nodes"] == 2).all()
        assert (o["ids"][:, 0] != -2).all() and (o["ids"][:, 1:] == -2).all() and (o["best"] == o["ids"][:, 0]).all()
        assert (o["value"][:, 0] <= Rn).all() and not o["value"][:, 1:].any()


def test_nothing_written_and_repeatable():
    st, tcount = _positions()
    bb = blokus_batch(st, FIRST_ENV_ID, tcount)
    fields = ("occ", "inv", "score", "round", "to_move", "tcount")
    before = [np_of(getattr(bb, k)).copy() for k in fields]
    for Rn, cand in ((1, None), (5, to_dev(_candidates()))):
        first = _run(bb, S, Rn, cand, W, SEED)
        again = _run(bb, S, Rn, cand, W, SEED)
        assert all(np.array_equal(first[k], again[k]) for k in KEYS)
        assert all(np.array_equal(first[k], _gpu(Rn, cand is not None)[k]) for k in KEYS)
    assert all(np.array_equal(a, np_of(getattr(bb, k))) for a, k in zip(before, fields))


def test_placement_independence():
    """a position gives the same row wherever it sits in the batch, when first_env_id is shifted to keep its game id"""
    st, tcount = _positions()
    pad = 3
    wide = BP.concat([BP.clone(st, [2] * pad), st])
    bb = blokus_batch(wide, FIRST_ENV_ID - pad, np.concatenate([np.full(pad, 77, np.uint32), tcount]))
    for Rn in (1, 5):
        o = _run(bb, S, Rn, None, W, SEED)
        assert all(np.array_equal(o[k][pad:], _gpu(Rn, False)[k]) for k in KEYS)


def test_invariants_on_a_batch():
    """what any such tree has, without the restatement: 64 mid-game positions, S = 200, R = 1, W = 8"""
    import torch
    from oracle import oracle as O
    B, S_, W_, Rn = 64, 200, 8, 1
    st = O.BlokusState(B)
    O.blokus_rollout(st, 77, 9100, 28, n_threads=BP.THREADS)
    assert not st.n_episodes.any()
    bb = blokus_batch(BP.clone(st), 9100)
    o = _run(bb, S_, Rn, None, W_, 12, 1.0)
    n_legal = np_of(bb.valid())
    assert n_legal.min() >= 0 and n_legal.max() > W_
    assert (o["visits"].sum(axis=1) == S_).all() and (o["nodes"] <= S_ + 1).all() and (o["nodes"] >= 2).all()
    n_children = (o["ids"] != -2).sum(axis=1)
    assert (n_children == np.minimum(np.minimum(W_, np.maximum(n_legal, 1)), math.isqrt(S_ - 1) + 1)).all()
    assert (o["value"] <= o["visits"] * Rn).all()
    for k in range(W_):
        col = o["ids"][:, k]
        has = col != -2
        assert (has == (k < n_children)).all() and (o["visits"][~has, k] == 0).all() and (o["visits"][has, k] >= 1).all()
        ok = np_of(bb.is_valid(torch.from_numpy(np.where(col >= 0, col, 0).astype(np.int32)).to(DEV)))
        assert ((ok == 1) | (col < 0)).all() and ((col != -1) | (n_legal == 0)).all()
    for b in range(B):
        kids = o["ids"][b, :n_children[b]].tolist()
        assert len(set(kids)) == len(kids)
        top = [k for k in range(n_children[b]) if o["visits"][b, k] == o["visits"][b].max()]
        assert o["best"][b] == o["ids"][b, min(k for k in top if o["value"][b, k] == max(o["value"][b, t] for t in top))]


def test_forced_win():
    """An endgame of blokus_positions.late ("ends": whatever the mover plays ends the game) in which the mover is then alone
    on top.  A ply ends the game iff nobody -- the mover's remaining pieces included -- has an action on the board before
    it, so at one position either every legal action ends the game or none does: the columns beside the winning one are
    a dense id that is not legal, a pass and a repeat.  With cexp = 0 `best` is the winning candidate, every simulation
    goes through it and every playout is the mover's; with a widening root every child is such a win."""
    from oracle import oracle as O
    late = BP.late(24)
    found = None
    for b in np.flatnonzero(BP.late_kinds(late)[1]):
        one = blokus_one(late, int(b))
        legal = [int(i) for i in blokus_list(one)]
        mover = int(one.to_move[0]) & 3
        if not legal:
            continue
        _, term, ws = O.blokus_step(one, np.array([legal[-1]], np.int32))
        if term[0] and int(ws[0]) == 1 << mover:
            found = (int(b), legal)
            break
    assert found is not None
    b, legal = found
    illegal = next(i for i in range(336000) if i not in set(legal))
    bb = blokus_batch(BP.clone(late, [b]), 31)
    for Rn in (1, 5):
        o = _run(bb, 12, Rn, to_dev(np.array([[illegal, legal[-1], -1, legal[-1]]], np.int32)), 4, 3, 0.0)
        assert o["best"][0] == legal[-1] and o["ids"][0].tolist() == [-2, legal[-1], -2, -2]
        assert o["visits"][0, 1] == 12 and o["value"][0, 1] == 12 * Rn and o["nodes"][0] == 2
        o = _run(bb, 12, Rn, None, 4, 3, 0.0)
        assert o["best"][0] in legal and (o["value"][0] == o["visits"][0] * Rn).all() and o["visits"][0].sum() == 12


def test_env_mcts_action():
    """BlokusSinglePlayerVectorEnv.mcts_action is batch.mcts_action on the env's position, and stepping with it stays legal"""
    import torch
    from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv
    env = BlokusSinglePlayerVectorEnv(batch=8, seat=torch.tensor([0, 1, 2, 3, 0, 1, 2, 3], dtype=torch.int8, device=DEV), seed=3,
                                      device=DEV)
    env.reset()
    for t in range(3):
        act = env.mcts_action(16, 1, 4, seed=9 + t)
        assert act.dtype == torch.int64 and tuple(act.shape) == (8,)
        assert torch.equal(act, env.batch.mcts_action(16, 1, None, 4, 9 + t, 1.0))
        assert (np_of(env.batch.to_move) & 3 == np_of(env.seat)).all()                  # the searched mover is the learner
        a, n_valid = np_of(act), np_of(env.batch.valid())
        ok = np_of(env.batch.is_valid(act.clamp(min=0).to(torch.int32)))
        assert (((a >= 0) & (ok == 1)) | ((a == -1) & (n_valid == 0))).all()
        _, reward, _, _ = env.step(act)
        assert (np_of(reward) >= 0).all()                                               # no CRL_BLOKUS_*_ERROR code
