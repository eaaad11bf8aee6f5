"""The whole TicTacToe search with the packed MLP in one launch (crl_ttt_puct_search, TTTBatch.puct_search / puct_net):
1. byte for byte what the three-launch loop leaves -- the whole tree buffers and every root output -- over the shapes, network
   widths, batch sizes and simulation counts at which the kernel takes another path;
2. against the same network in float64 numpy at the two smallest shapes: the root's priors after one simulation, the visited
   child's value after two.  Bounds (derived, not measured): crl_ttt_net_eval is held to 4 units on its max-scaled priors q
   (sum >= 65535), so a prior p normalised to 65536 over n_e empty cells may differ by 4 + 4 n_e p / 65535 + 2 (the 2: the
   floor of the division and the rounding of the reference); a value by the existing 4 units.
   Largest deviation measured on an MI355X: prior 1.48 (bounds 6 .. 91), value 0.50;
3. captured into a graph and replayed; 4. through puct_net_action."""
import functools

import numpy as np
import pytest
import torch

from colosseumrl_amd.batched import TTTBatch
from tests.gpu_util import DEV, np_of as _np

pytestmark = pytest.mark.gpu
ROOT_KEYS = ("visits", "value", "prior", "nodes", "sims", "best")
SHAPES = {"3x3": ((3, 3), 3, 2), "3x5": ((3, 5), 3, 3), "3x3x3": ((3, 3, 3), 3, 4), "5x5": ((5, 5), 4, 3)}
GRID = 16 * 512                                                  # trees in one pass of the grid
# shape, H, L, planes, B, S, random plies before the search (enough for finished games and terminal leaves)
CASES = [("3x3", 16, 1, None, 1, 1, 3), ("3x3", 16, 1, None, 17, 64, 7), ("3x3", 16, 1, 1, GRID + 17, 4, 5),
         ("3x5", 48, 2, None, 17, 64, 7), ("3x5", 256, 3, 1, 33, 2, 7), ("3x3x3", 256, 3, None, 17, 2, 9),
         ("3x3x3", 48, 2, 1, 40, 64, 9), ("5x5", 256, 3, None, 17, 64, 12), ("5x5", 16, 1, None, 1, 2, 12)]


def _network(rng, cells, P, C, H, L):
    """weights N(0, 9 / fan_in) and biases N(0, 1), rounded to float32: [(W, b)] of the hidden layers, the policy and the value head"""
    dims = [(H, cells * C)] + [(H, H)] * (L - 1) + [(cells, H), (P, H)]
    return [((rng.standard_normal(d) * 3.0 / np.sqrt(d[1])).astype(np.float32), rng.standard_normal(d[0]).astype(np.float32)) for d in dims]


def _pack(tb, layers, C=None):
    dev = [(torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)) for W, b in layers]
    return tb.net_pack(dev[:-2], dev[-2], dev[-1], C)


def _twins(shape, H, L, planes, B, cap, plies, seed=3):
    """two batches in the same positions after `plies` random plies, each with its packed copy of one network and zeroed trees"""
    dims, k, P = SHAPES[shape]
    layers = _network(np.random.default_rng(seed), int(np.prod(dims)), P, planes or P, H, L)
    out = []
    for _ in range(2):
        tb = TTTBatch(dims, k, P, B, device=DEV)
        for s in range(plies):
            tb.step(tb.sample(seed=11))
        tb.puct_begin(cap)
        tb._puct_tree.zero_()                                    # (torch.empty: the nodes no search reaches would differ)
        tb.puct_begin(cap)
        out.append((tb, _pack(tb, layers, planes)))
    return out


def _loop(tb, net, S, rel_mod=None):
    leaves = out = None
    for _ in range(S):
        leaves = tb.puct_select(rel_mod=rel_mod, out=leaves)
        out = tb.net_eval(net, leaves, out=out)
        tb.puct_backup(*out)


def _same(a, b, what):
    assert torch.equal(a._puct_tree, b._puct_tree), (what, "trees", int((a._puct_tree != b._puct_tree).any(dim=(1, 2)).sum()))
    ra, rb = a.puct_root(), b.puct_root()
    for key in ROOT_KEYS:
        assert torch.equal(ra[key], rb[key]), (what, key)
    return ra


@pytest.mark.parametrize("shape, H, L, planes, B, S, plies", CASES, ids=["%s_h%d_l%d_c%s_b%d_s%d" % c[:6] for c in CASES])
def test_equal_to_the_loop(shape, H, L, planes, B, S, plies):
    (a, net_a), (b, net_b) = _twins(shape, H, L, planes, B, S, plies)
    want, got = a.puct(net_a.evaluator(), S), b.puct_net(net_b, S)
    for key in ROOT_KEYS:
        assert torch.equal(want[key], got[key]), key
    root = _same(a, b, shape)
    live = _np(root["nodes"]) > 0
    assert (_np(root["sims"])[live] == S).all()
    if B == 17 and shape == "3x3":
        assert 0 < live.sum() < B                                # skipped trees among the running ones


@pytest.mark.parametrize("how", ["twice", "interleaved", "past_capacity"])
def test_continued_searches(how):
    """3x5 for three players with rel_mod = 2: two calls against one loop; a triple of the three launches between two calls;
    n_sims past S_cap"""
    cap = {"twice": 64, "interleaved": 64, "past_capacity": 24}[how]
    (a, net_a), (b, net_b) = _twins("3x5", 48, 2, 2, 19, cap, 6)
    _loop(a, net_a, 64, rel_mod=2)
    if how == "interleaved":
        b.puct_search(net_b, 40, rel_mod=2)
        _loop(b, net_b, 1, rel_mod=2)
        b.puct_search(net_b, 23, rel_mod=2)
    else:
        b.puct_search(net_b, 40, rel_mod=2)
        b.puct_search(net_b, 24, rel_mod=2)
    root = _same(a, b, how)
    assert (_np(root["sims"])[_np(root["nodes"]) > 0] == cap).all()


# ------------------------------------------------------------------ 2. against float64
def _positions(shape, B, seed):
    """host-made positions two plies into the game (no game is over, every root differs): occ uint32 [P, B], the mover"""
    dims, k, P = SHAPES[shape]
    rng, cells = np.random.default_rng(seed), int(np.prod(dims))
    picks = np.array([rng.permutation(cells)[:2] for _ in range(B)])
    occ = np.zeros((P, B), np.uint32)
    occ[0], occ[1] = np.uint32(1) << picks[:, 0].astype(np.uint32), np.uint32(1) << picks[:, 1].astype(np.uint32)
    return occ, 2 % P


def _forward(layers, C, board):
    x = (board[:, :, None] == np.arange(C)).reshape(len(board), -1).astype(np.float64)
    for W, b in layers[:-2]:
        x = np.maximum(x @ W.astype(np.float64).T + b, 0.0)
    (Wp, bp), (Wv, bv) = layers[-2:]
    return x @ Wp.astype(np.float64).T + bp, x @ Wv.astype(np.float64).T + bv


def _relative(occ, mover, cells, P):
    owner = np.full((occ.shape[1], cells), -1, np.int64)
    for p in range(P):
        owner[((occ[p][:, None] >> np.arange(cells, dtype=np.uint32)) & 1) == 1] = p
    return np.where(owner < 0, -1, (owner - mover) % P)


@functools.lru_cache(maxsize=None)
def _float64_case(shape, B=64, seed=2):
    """the reference alone (no GPU): root priors on 0 .. 65536, their bound, the decided trees, the value of their first child"""
    dims, k, P = SHAPES[shape]
    cells = int(np.prod(dims))
    layers = _network(np.random.default_rng(seed), cells, P, P, 32, 2)
    occ, mover = _positions(shape, B, seed)
    board = _relative(occ, mover, cells, P)
    logit, _ = _forward(layers, P, board)
    logit = np.where(board < 0, logit, -np.inf)
    e = np.exp(logit - logit.max(axis=1, keepdims=True))
    prior = 65536.0 * e / e.sum(axis=1, keepdims=True)
    n_e = (board < 0).sum(axis=1, keepdims=True)
    bound = 4.0 + 4.0 * n_e * prior / 65535.0 + 2.0
    order = np.argsort(prior, axis=1)
    first, second = order[:, -1], order[:, -2]
    rows = np.arange(B)
    decided = prior[rows, first] - prior[rows, second] > 2.0 * bound[rows, first]
    child = occ.copy()
    child[mover, rows] |= np.uint32(1) << first.astype(np.uint32)
    _, v = _forward(layers, P, _relative(child, (mover + 1) % P, cells, P))
    value = 65536.0 / (1.0 + np.exp(-v[:, P - 1]))               # of who moved in, seen from the child's mover: the last in turn order
    return layers, occ, mover, prior, bound, decided, first, value


@pytest.mark.parametrize("shape", ["3x3", "3x3x3"])
def test_against_float64(shape):
    dims, k, P = SHAPES[shape]
    layers, occ, mover, prior, bound, decided, first, value = _float64_case(shape)
    B = occ.shape[1]
    assert decided.mean() >= 0.75
    tb = TTTBatch(dims, k, P, B, device=DEV)
    tb.occ.copy_(torch.from_numpy(occ.view(np.int32)))
    tb.to_move.fill_(mover)
    net = _pack(tb, layers)
    got = _np(tb.puct_net(net, 1)["prior"]).astype(np.float64)
    print("%s: largest prior deviation %.2f (bound %.2f .. %.2f)" % (shape, np.abs(got - prior).max(), bound.min(), bound.max()))
    assert (np.abs(got - prior) <= bound).all()
    root = {key: _np(t) for key, t in tb.puct_net(net, 2).items()}
    rows = np.arange(B)[decided]
    assert (root["visits"][rows, first[rows]] == 1).all() and (root["visits"].sum(axis=1) == 1).all()
    dv = np.abs(root["value"][rows, first[rows]] - value[rows])
    print("%s: largest value deviation %.2f over %d of %d trees" % (shape, dv.max(), len(rows), B))
    assert (dv <= 4.0).all()


# ------------------------------------------------------------------ 3. under a graph, 4. through the product
def test_graph_replays_equal_the_eager_calls():
    (a, net_a), (b, net_b) = _twins("3x5", 48, 2, None, 21, 9, 6)
    for _ in range(3):
        a.puct_search(net_a, 3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on a side stream, as torch.cuda.graph wants
        b.puct_search(net_b, 3)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.puct_search(net_b, 3)
    for done in (6, 9):                                          # (the warm-up ran three simulations, a capture runs nothing)
        g.replay()
        torch.cuda.synchronize()
        assert (_np(b.puct_root()["sims"]).max()) == done
    _same(a, b, "graph")


def test_puct_net_action():
    (a, net_a), (b, net_b) = _twins("3x3x3", 48, 2, None, 23, 16, 9)
    want, got = a.puct_action(net_a.evaluator(), 16), b.puct_net_action(net_b, 16)
    assert got.dtype == torch.int64 and torch.equal(want, got) and (got >= 0).any()
