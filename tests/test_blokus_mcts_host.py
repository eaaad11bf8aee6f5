"""The Blokus tree search (crl_blokus_mcts) on the host: the argument checks of the two C entries (every CRL_EINVAL case is
refused with its message before any device work), S_max, the argument checks of the Python wrappers, the counter-space
separation from crl_blokus_playout, and the properties of the plain-Python restatement (tests/blokus_mcts_ref.py) on two
small positions."""
import math

import numpy as np
import pytest

from tests import blokus_mcts_ref as M
from tests import rng_ref as RNG
from tests.host_util import D, fake as _fake, lib as _lib, refused, ttt_context

S_MAX = 1823


def _call(lib, ctx=None, B=4, state=(D,) * 6, cand=None, A=1, W=8, S=8, Rn=1, cexp=256, outs=(D,) * 5, flags=0):
    return lib.crl_blokus_mcts(ctx, B, 1, 0, *state, cand, A, W, S, Rn, cexp, *outs, flags, None)


def test_argument_checks():
    """no Blokus context can be made without a device, so the context check, which comes last, ends every good call"""
    lib = _lib()
    for i in range(5):                     # occ, inv, score, round, to_move (tcount may be NULL)
        st = [D] * 6
        st[i] = None
        refused(lib, _call(lib, state=tuple(st)), b"crl_blokus_mcts", b"NULL state")
    st = [D] * 6
    st[5] = None
    refused(lib, _call(lib, state=tuple(st)), b"blokus context")
    for i in range(5):
        outs = [D] * 5
        outs[i] = None
        refused(lib, _call(lib, outs=tuple(outs)), b"NULL output")
    for B in (0, -1, (1 << 28) + 1):
        refused(lib, _call(lib, B=B), b"B=")
    for A in (0, 65, -1):
        refused(lib, _call(lib, cand=D, A=A), b"A=")
    for A in (0, 2, 64):
        refused(lib, _call(lib, cand=None, A=A), b"A=", b"cand")
    refused(lib, _call(lib, cand=D, A=64), b"blokus context")
    for W in (0, 65, -8):
        refused(lib, _call(lib, W=W), b"W=")
    for S in (0, -1, S_MAX + 1, 65536, 1 << 30):
        refused(lib, _call(lib, S=S), b"S=")
    for Rn in (0, -3, 1025, 65535):
        refused(lib, _call(lib, Rn=Rn), b"R=")
    for cexp in (65536, 0xFFFFFFFF):
        refused(lib, _call(lib, cexp=cexp), b"cexp=")
    for flags in (1, 8, 0x80000000):
        refused(lib, _call(lib, flags=flags), b"flags")
    refused(lib, _call(lib), b"blokus context")
    assert lib.crl_blokus_mcts_max_simulations(None) == -1 and b"blokus context" in lib.crl_last_error()
    with ttt_context() as tt:              # a context of another game
        refused(lib, _call(lib, ctx=tt), b"blokus context")
        assert lib.crl_blokus_mcts_max_simulations(tt) == -1 and b"blokus context" in lib.crl_last_error()


def test_max_simulations():
    """S_max = min(65535, (45056 - 1280) / 24 - 1): a tree of S_max + 1 nodes and its fixed part fill the 45,056 bytes a
    workgroup's trees get; S_max passes the check of S (the call is stopped by a later check, so nothing is launched),
    S_max + 1 does not."""
    lib = _lib()
    assert M.S_MAX == S_MAX == min(65535, (45056 - 1280) // 24 - 1) and S_MAX >= 511
    assert (S_MAX + 1) * 24 + 1280 <= 45056 < (S_MAX + 2) * 24 + 1280
    assert 2 * min(S_MAX, M.MAX_DEPTH) + 2 <= 1280             # the path fits the fixed part
    refused(lib, _call(lib, S=S_MAX, flags=1), b"flags")
    refused(lib, _call(lib, S=S_MAX), b"blokus context")
    refused(lib, _call(lib, S=S_MAX + 1, flags=1), b"S=")


def test_prototypes_abi_and_tags():
    import os
    import re
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    assert "crl_blokus_mcts" in _native.PROTOTYPES and "crl_blokus_mcts_max_simulations" in _native.PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = open(os.path.join(root, "colosseumrl_amd", "csrc", "crl_common.hpp")).read()
    assert len(re.findall(r"#define\s+CRL_TAG_\w+", common)) == 12       # the search has no tag of its own
    assert M.TAG == 0x42500000


def test_draw_words_differ_from_the_playout_entry():
    """crl_blokus_playout's second counter word is c >> 2 < 2^30; the search sets bit 30 or bit 31 there, so for the same
    (g, c) and third word the blocks -- hence the words -- differ"""
    from tests.blokus_ref import blokus_word
    rng = np.random.default_rng(11)
    for _ in range(50):
        seed, g, c = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))
        s, r = int(rng.integers(0, S_MAX)), int(rng.integers(0, 1024))
        entry = blokus_word(seed, g, c, (s << 16) | r, RNG.CRL_TAG_BLOKUS_PLAYOUT)
        assert M.playout_word(seed, g, c, s, r) != entry
        assert M.widen_word(seed, g, c & 0x1ff, s) != int(RNG.philox(g, c & 0x1ff, s, M.TAG, seed)[0])
    assert all(((c >> 2) | M.PLAYOUT_BIT) >= 2 ** 30 > (c >> 2) for c in (0, 5, 2 ** 32 - 1))
    assert all((M.WIDEN_BIT | d) >= 2 ** 31 > ((c >> 2) | M.PLAYOUT_BIT) for d in (0, 336) for c in (0, 2 ** 32 - 1))


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv
    bb = _fake(BlokusBatch, B=3, P=4)
    bb.__dict__["mcts_max_simulations"] = S_MAX
    i32 = torch.int32
    ok = torch.zeros((3, 5), dtype=i32)
    for fn in (bb.mcts, bb.mcts_action):
        for bad in (0, S_MAX + 1, -1, 2.0, True, None):
            with pytest.raises(ValueError):
                fn(bad)
        for bad in (0, 1025, 16.0, False):
            with pytest.raises(ValueError):
                fn(8, bad)
        for cand in (torch.zeros((3, 5), dtype=torch.int64), torch.zeros((2, 5), dtype=i32), torch.zeros((3,), dtype=i32),
                     torch.zeros((3, 65), dtype=i32), torch.zeros((3, 0), dtype=i32), np.zeros((3, 5), np.int32)):
            with pytest.raises(ValueError):
                fn(8, 1, cand)
        for bad in (0, 65, 8.0, True):
            with pytest.raises(ValueError):
                fn(8, 1, None, bad)
        for bad in (-0.5, 256.0, float("nan"), "1", True, None):
            with pytest.raises(ValueError):
                fn(8, 1, None, 8, 0, bad)
    good = {"ids": torch.zeros((3, 8), dtype=i32), "visits": torch.zeros((3, 8), dtype=i32), "value": torch.zeros((3, 8), dtype=i32),
            "nodes": torch.zeros((3,), dtype=i32), "best": torch.zeros((3,), dtype=i32)}
    for key, wrong in (("ids", torch.zeros((3, 5), dtype=i32)), ("visits", torch.zeros((3, 8), dtype=torch.int64)),
                       ("value", torch.zeros((2, 8), dtype=i32)), ("nodes", torch.zeros((4,), dtype=i32)),
                       ("best", torch.zeros((3,), dtype=torch.int64))):
        with pytest.raises(ValueError):
            bb.mcts(8, out=dict(good, **{key: wrong}))
        with pytest.raises(ValueError):
            bb.mcts(8, out={k: v for k, v in good.items() if k != key})
    with pytest.raises(ValueError):        # with candidates K = A, not the width
        bb.mcts(8, candidates=ok, out=good)
    env = _fake(BlokusSinglePlayerVectorEnv, batch=bb, rank=True)
    with pytest.raises(ValueError):        # the search answers with dense ids
        env.mcts_action(8)
    env.rank = False
    for args in ((0,), (8, 0), (8, 1, 65), (8, 1, 8, 1, -1.0)):
        with pytest.raises(ValueError):
            env.mcts_action(*args)


# ---- the restatement: its parts and the properties any such tree has
def test_score_parts():
    assert all(M.lg(1 << k) == 256 * k for k in range(32)) and M.lg(3) == 256 + 128 and M.lg(511) == 256 * 8 + 255
    assert M.score(7, 3, 3 * 16, 16, 0) == 65536 and M.score(9, 2, 0, 5, 0) == 0 and M.score(9, 2, 5, 5, 0) == 32768
    assert M.score(4, 1, 0, 1, 256) == 92681                    # n_v = 4, n_u = 1: isqrt(512 << 24)
    assert M.score(S_MAX, 1, 1024, 1024, 65535) < 1 << 27        # the greatest score there is
    assert [M.cexp_of(v) for v in (0, 1.0, 0.5)] == [0, 256, 128]


@pytest.fixture(scope="module")
def small_positions():
    """two positions with cheap playouts: a round-6 board with inventories of one or two pieces whose mover has a choice,
    and one late in a real game whose mover must pass while another player can move"""
    from tests import blokus_positions as BP
    tiny, late = BP.tiny_inventories(12), BP.late(24)
    n_legal = BP.counts(tiny)[np.arange(tiny.B), tiny.to_move & 3]
    a = int(np.flatnonzero(n_legal >= 6)[0])
    b = int(np.flatnonzero(BP.late_kinds(late)[0] >= 1)[0])
    return BP.concat([BP.clone(tiny, [a]), BP.clone(late, [b])])


def test_tree_properties(small_positions):
    from tests.blokus_ref import blokus_list, blokus_one
    st = small_positions
    before = [getattr(st, name).copy() for name in ("occ", "inv", "score", "round", "to_move")]
    Rn = 2
    for S, W in ((1, 4), (10, 4), (17, 8)):
        ids, visits, value, nodes, best = M.blokus_mcts(st, S, Rn, W, 256, seed=5, first_env_id=3, tcount=np.array([7, 2 ** 32 - 2]))
        again = M.blokus_mcts(st, S, Rn, W, 256, seed=5, first_env_id=3, tcount=np.array([7, 2 ** 32 - 2]))
        assert all(np.array_equal(x, y) for x, y in zip((ids, visits, value, nodes, best), again))   # the same inputs, the same tree
        assert all(np.array_equal(x, getattr(st, name)) for x, name in zip(before, ("occ", "inv", "score", "round", "to_move")))
        for b in range(st.B):
            legal = [int(i) for i in blokus_list(blokus_one(st, b))]
            cap = min(W, max(len(legal), 1))
            n_children = int((ids[b] != -2).sum())
            assert visits[b].sum() == S and n_children == min(cap, math.isqrt(S - 1) + 1)
            assert (ids[b, :n_children] != -2).all() and (visits[b, n_children:] == 0).all() and (value[b, n_children:] == 0).all()
            kids = [int(i) for i in ids[b, :n_children]]
            assert len(set(kids)) == len(kids) and (set(kids) <= set(legal) if legal else kids == [-1])
            assert (value[b] <= visits[b] * Rn).all() and 2 <= nodes[b] <= S + 1
            top = [k for k in range(n_children) if visits[b, k] == visits[b].max()]
            assert best[b] == ids[b, min(k for k in top if value[b, k] == max(value[b, t] for t in top))]


def test_candidate_root(small_positions):
    from tests.blokus_ref import blokus_list, blokus_one
    st = small_positions
    legal = [int(i) for i in blokus_list(blokus_one(st, 0))]
    illegal = next(i for i in range(336000) if i not in set(legal))
    cand = np.array([[legal[4], illegal, legal[1], legal[4], -1], [illegal, -1, 336000, illegal, -1]])
    ids, visits, value, nodes, best = M.blokus_mcts(st, 9, 1, 4, 256, seed=1, cand=cand)
    assert ids[0].tolist() == [legal[4], -2, legal[1], -2, -2] and visits[0].sum() == 9 and (visits[0, [1, 3, 4]] == 0).all()
    assert visits[0, 0] >= 1 and visits[0, 2] >= 1 and best[0] in (legal[4], legal[1]) and nodes[0] <= 10
    assert ids[1].tolist() == [-2] * 5 and not visits[1].any() and not value[1].any() and nodes[1] == 0 and best[1] == -2   # skipped
