"""The Blokus search valued by the caller's network on the GPU (crl_blokus_puct_*, BlokusBatch.puct_*): every `select` output
of every simulation and the `root` row bit for bit against the plain-Python restatement of the header's contract
(tests/blokus_puct_ref.py) on the positions of tests/blokus_mcts_cases.py at W = 1, 4, 8 and 64; the candidate pick alone
against valid_list and the ranks; a path longer than 64 nodes; tree offsets past 2^32 bytes; the pair captured into a graph;
the refusals; and a puct_action learner valued by playouts next to a random learner."""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import blokus_mcts_cases as CASES
from tests import blokus_positions as BP
from tests import blokus_puct_ref as R
from tests.gpu_util import DEV, blokus_batch, np_of, u32_of

pytestmark = pytest.mark.gpu
S_CAP, CPUCT, FPU = 24, 320, 32768
UNSIGNED = ("leaf_occ", "leaf_inv")


@functools.lru_cache(maxsize=None)
def _rows():
    """the empty board, tiny0, tiny11, late8, must_pass, finished and the capped rows L = 1, 2, 4, 6, 8: (state, tcount, id)"""
    five, capped = CASES.rows("five"), CASES.rows("capped")
    st = BP.concat([O.BlokusState(1), five.state, capped.state])
    return st, np.concatenate([np.array([7], np.uint32), five.tcount, capped.tcount]), CASES.ID_BASE + 4500


def _leaves_np(leaves):
    return {k: (u32_of(v) if k in UNSIGNED else np_of(v)) for k, v in leaves.items()}


def _same(got, want, what):
    for key, w in want.items():
        g = got[key].astype(w.dtype) if key in R.ROOT_KEYS else got[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, key, np.argwhere(g != w)[:6].tolist())


def _backup(bb, leaves):
    prior, value = R.evaluator(leaves)
    bb.puct_backup(prior.to(torch.int16), value.to(torch.int32))


@functools.lru_cache(maxsize=None)
def _reference(W, S=S_CAP + 2):
    """the restatement's select outputs of S simulations (the last two at capacity) and its root, computed once"""
    st, tcount, first = _rows()
    ref = R.Search(st, S_CAP, W, CASES.SEED, first, tcount)
    seen = []
    for _ in range(S):
        seen.append(ref.select(CPUCT, FPU))
        prior, value = R.evaluator(seen[-1])
        ref.backup(prior, value)
    return seen, ref.root()


@pytest.mark.parametrize("W", (1, 4, 8, 64))
def test_matches_the_restatement(W):
    st, tcount, first = _rows()
    want_seen, want_root = _reference(W)
    bb = blokus_batch(st, first, tcount)
    bb.puct_begin(S_CAP, W, CASES.SEED)
    bb.step_observe(seed=3)                                      # the trees hold their own copy: the batch may move on
    leaves = None
    for s, want in enumerate(want_seen):
        again = _leaves_np(bb.puct_select(CPUCT / 256, FPU / 65536))
        leaves = bb.puct_select(CPUCT / 256, FPU / 65536, out=leaves)
        got = _leaves_np(leaves)
        _same(got, again, ("select twice", s))                   # without a backup: the same leaf
        _same(got, want, ("select", s))
        _backup(bb, leaves)
    assert not want_seen[-1]["pending"].any() and want_seen[S_CAP - 1]["pending"].any()      # at capacity: pending 0
    _same(_leaves_np(bb.puct_root()), want_root, "root")
    assert int(np_of(bb.puct_root()["sims"]).max()) == S_CAP


@pytest.mark.parametrize("W", (8, 10, 11, 64))                 # (up to 10 candidates the pick walks ranks, above it enumerates)
def test_the_pick_is_the_ranked_actions_of_valid_list(W):
    from colosseumrl_amd.batched import BlokusBatch
    st, tcount, first = _rows()
    board = np.zeros((3, 20, 20), np.int8)                       # the lattices of test_blokus_valid_list_more_than_128_anchors: ~170 anchors
    board[0, 1::3, 1::3], board[1, 0::3, 0::3], board[2, 1::3, 1::3] = 1, 2, 3
    board[2, 2::6, 2::6] = 1
    for bb, tc, name in ((blokus_batch(st, first, tcount), tcount, "rows"), (BlokusBatch(3, device=DEV, first_env_id=first), None, "lattice")):
        if name == "lattice":
            bb.set_board(torch.from_numpy(board).to(DEV))
            bb.round.fill_(5)
            bb.to_move.copy_(torch.arange(3, dtype=torch.int32))
            tc = np.zeros(3, np.uint32)
        count, ids = (np_of(t) for t in bb.valid_list(65536))
        bb.puct_begin(4, W, CASES.SEED)
        got = _leaves_np(bb.puct_select())
        assert (got["n_legal"] == count).all() and count.max() <= 65536 and (name == "rows" or (count > W).all())
        for b in range(bb.B):
            L = int(count[b])
            want = [int(ids[b, r]) for r in R.ranks(L, W, CASES.SEED, (first + b) & 0xFFFFFFFF, int(tc[b]), 0)] if L else [-1]
            assert got["cand"][b].tolist() == want + [-2] * (W - len(want)), (name, b, L)


def test_a_path_longer_than_64_nodes():
    """W = 1 from the empty board: the tree is a chain that grows a ply per simulation, and backup walks it 64 nodes a pass"""
    st, S = O.BlokusState(1), 76                                 # (game id 4020: of 4000 .. 4029 the longest chain, 75 nodes)
    tcount, first = np.array([5], np.uint32), CASES.ID_BASE + 4020
    ref = R.Search(st, S, 1, CASES.SEED, first, tcount)
    bb = blokus_batch(st, first, tcount)
    bb.puct_begin(S, 1, CASES.SEED)
    for s in range(S):
        want = ref.select(0, 0)
        leaves = bb.puct_select(0.0, 0.0)
        _same(_leaves_np(leaves), want, ("select", s))
        ref.backup(*R.evaluator(want))
        _backup(bb, leaves)
    assert len(ref.trees[0].nodes) >= 66                                   # a condition of the test: the last paths are 65 nodes and more
    _same(_leaves_np(bb.puct_root()), ref.root(), "root")


def test_tree_offsets_past_4_gib():
    """S_cap = 4095, W = 64: a tree is 2.1 MB, so the trees from 2,001 on lie past 2^32 bytes.  Every row holds the same
    position (L > W there, so the game id enters the candidates); a row must end as the one-tree run with its game id."""
    from colosseumrl_amd.batched import BlokusBatch
    B, S = 2051, 5
    src = BlokusBatch(1, device=DEV)
    for _ in range(4):
        src.step_observe(seed=1)

    def run(n, first):
        bb = BlokusBatch(n, device=DEV, first_env_id=first)
        for name in ("occ", "inv", "score", "round", "to_move", "tcount"):
            getattr(bb, name).copy_(getattr(src, name).expand_as(getattr(bb, name)))
        bb.puct_begin(4095, 64, 3)
        for _ in range(S):
            _backup(bb, bb.puct_select())
        return bb, _leaves_np(bb.puct_root())
    big, got = run(B, 9)
    assert big._puct_tree.numel() * 8 > 2 ** 32 and (got["sims"] == S).all()
    for b in (0, 2000, 2001, B - 1):
        _same({k: v[b:b + 1] for k, v in got.items()}, run(1, 9 + b)[1], ("row", b))
    assert not np.array_equal(got["ids"][0], got["ids"][B - 1])  # the game id did enter


def test_graph_replay_equals_the_eager_run():
    st, tcount, first = _rows()
    S, W = 12, 8
    eager = blokus_batch(st, first, tcount)
    evaluate = lambda leaves: tuple(t.to(dt) for t, dt in zip(R.evaluator(leaves), (torch.int16, torch.int32)))
    want = _leaves_np(eager.puct(evaluate, S, W, seed=5))
    bb = blokus_batch(st, first, tcount)
    bb.puct_begin(S, W, 5)
    leaves = bb.puct_select()

    def pair():
        bb.puct_select(out=leaves)
        bb.puct_backup(*evaluate(leaves))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on a side stream, as torch.cuda.graph wants
        pair()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                    # one stream, one chain: no parallel branches
        pair()
    bb.puct_begin(S, W, 5)                                       # the warm-up was a simulation: start again
    for _ in range(S):
        g.replay()
    torch.cuda.synchronize()
    _same(_leaves_np(bb.puct_root()), want, "graph")


@pytest.mark.parametrize("what", ["tree_null", "tree_unaligned", "B", "S_cap_0", "S_cap_4096", "W_0", "W_65", "cpuct", "fpu", "flags_select",
                                  "flags_backup", "null_out", "null_state", "leaf_partial", "null_prior", "null_root", "ctx"])
def test_refusals(what):
    import ctypes
    from colosseumrl_amd.batched import TTTBatch, _ptr
    bb = blokus_batch(O.BlokusState(2))
    bb.puct_begin(4, 4)
    lib, ctx, tree = bb._lib, bb._ctx.handle, _ptr(bb._puct_tree)
    if what == "ctx":
        ctx = TTTBatch((3, 3), 3, 2, 2, device=DEV)._ctx.handle
    o, r = bb.puct_select(), bb.puct_root()
    prior, value = torch.zeros((2, 4), dtype=torch.int16, device=DEV), torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    B, S_cap, W = 0 if what == "B" else 2, {"S_cap_0": 0, "S_cap_4096": 4096}.get(what, 4), {"W_0": 0, "W_65": 65}.get(what, 4)
    tree = {"tree_null": None, "tree_unaligned": ctypes.c_void_p(bb._puct_tree.data_ptr() + 8)}.get(what, tree)
    sel = [None if (what, k) in (("null_out", "cand"), ("leaf_partial", "leaf_round")) else _ptr(o[k]) for k in R.SELECT_KEYS]
    state = [None if what == "null_state" and i == 1 else p for i, p in enumerate(bb._state())]
    calls = {
        "begin": lambda: lib.crl_blokus_puct_begin(ctx, B, 0, 0, *state, None, S_cap, W, tree, None),
        "select": lambda: lib.crl_blokus_puct_select(ctx, B, tree, S_cap, W, 65536 if what == "cpuct" else 256, 65537 if what == "fpu" else 0,
                                                     *sel, 1 if what == "flags_select" else 0, None),
        "backup": lambda: lib.crl_blokus_puct_backup(ctx, B, tree, S_cap, W, None if what == "null_prior" else _ptr(prior), _ptr(value),
                                                     1 if what == "flags_backup" else 0, None),
        "root": lambda: lib.crl_blokus_puct_root(ctx, B, tree, S_cap, W, *[None if what == "null_root" and k == "best" else _ptr(r[k])
                                                                          for k in R.ROOT_KEYS], None)}
    only = {"cpuct": "select", "fpu": "select", "flags_select": "select", "null_out": "select", "leaf_partial": "select",
            "flags_backup": "backup", "null_prior": "backup", "null_root": "root", "null_state": "begin"}.get(what)
    for name, call in calls.items():
        if only in (None, name):
            assert call() == -1 and lib.crl_last_error(), (what, name)      # CRL_EINVAL, with a message
    if what in ("S_cap_0", "S_cap_4096", "W_0", "W_65", "ctx"):
        assert lib.crl_blokus_puct_tree_bytes(ctx, S_cap, W) == -1
    with pytest.raises(ValueError):
        bb.puct_begin(4096) if what != "W_65" else bb.puct_begin(4, 65)


def test_playout_valued_puct_learner_beats_the_random_learner():
    """128 games at seat 0, first episodes, against three random agents, as examples/blokus_puct.py plays them.  The learner plays
    puct_action(16, width=8) with uniform priors; the value of a leaf is the share of playout(4) each player won from the leaf_*
    state in a second stepper.  Its win share must exceed the uniformly random learner's on the same seeds by more than three
    standard errors of the difference of two binomials at the measured rates."""
    spec = importlib.util.spec_from_file_location("blokus_puct_example", os.path.join(os.path.dirname(__file__), "..", "examples", "blokus_puct.py"))
    EX = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(EX)
    G = 128
    evaluate = EX.playout_evaluator(G, 8, 4)
    torch.manual_seed(1)
    (puct, n_puct), (rand, n_rand) = (EX.play(G, 0, policy) for policy in (
        lambda env, t: env.puct_action(evaluate, 16, width=8, seed=1000 + t), EX.random_policy))
    assert n_puct == n_rand == G                                 # every game's first episode ended
    se = math.sqrt(puct * (1.0 - puct) / G + rand * (1.0 - rand) / G)
    print("\nfirst-episode win share over %d games: puct_action(16, width=8) valued by playout(4) %.4f, random learner %.4f, "
          "difference %.4f = %.1f standard errors" % (G, puct, rand, puct - rand, (puct - rand) / max(se, 1e-12)))
    assert puct - rand > 3.0 * se, (puct, rand, se)
