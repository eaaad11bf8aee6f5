"""The policy-value MLP of the Blokus search in one launch (crl_blokus_net_eval, BlokusBatch.net_pack / net_eval) against the
same network in float64 numpy, written from the header's words: at the shapes where the kernel takes another path (fewer output
tiles than waves, one to four tiles a wave, a k range that is no multiple of the four-tile chunk, one candidate slot and all
64) and B below a tile, with a ragged second tile, over many workgroups and past the grid (the grid-stride loop); then inside a
search and under a graph.  The reference's cell offsets come from the CPU oracle's step, not from the kernel's table.
Tolerance: 4 output units.  The same cases with the trunk and the heads in float32 by torch on the CPU differ from float64 by
at most 1 unit (prior) and 1 (value) over every case below, so the siblings' 4 units hold (the rule: 4 where that is at most 1,
else four times it).  The margin covers another summation order and the hardware exponential; an indexing or rotation error
moves priors by thousands.  Largest deviation measured on an MI355X over every case below and the search: prior 1, value 1."""
import functools

import numpy as np
import pytest
import torch

from colosseumrl_amd.batched import BlokusBatch
from tests.gpu_util import DEV, np_of as _np

pytestmark = pytest.mark.gpu
TOL = 4
SHAPES = [(16, 1, 1), (48, 3, 5), (128, 2, 16), (256, 2, 64)]                            # H, L, W
BLOCK_CAP = 1024                           # the kernel's workgroups per launch (BNET_MAX_BLOCKS), 16 leaves each and trip
CASES = [(s, B) for s in range(4) for B in (1, 17, 5000)] + [(0, BLOCK_CAP * 16 + 17)]  # the last: more tiles than the grid holds
IDS = 336000


@functools.lru_cache(maxsize=None)
def _offsets():
    """(cells [21, 8, 5, 5, 2]: the (dx, dy) from the anchor of the cells that (piece, orientation, shift) covers; count [21, 8,
    5]: how many, 0 where the shift names no cell of the piece), from the CPU oracle: each placement stepped onto the centre of an
    empty board and observed by player 0"""
    from oracle import oracle as O
    ids = np.arange(21 * 8 * 5)
    st = O.BlokusState(len(ids))
    O.blokus_step(st, O.blokus_encode(ids // 40, 10, 10, (ids // 5) % 8, ids % 5).astype(np.int32))
    board = O.blokus_observe(st, np.zeros(len(ids), np.int8))[0]
    cells, count = np.zeros((len(ids), 5, 2), np.int64), np.zeros(len(ids), np.int64)
    for k in ids:
        ys, xs = np.nonzero(board[k] == 0)                                          # player 0's frame: row y, column x
        cells[k, :len(xs)], count[k] = np.stack([xs - 10, ys - 10], axis=1), len(xs)
    assert count.reshape(21, 40)[:, 0].sum() == 89 and count.max() == 5             # the 21 pieces' cells
    return cells.reshape(21, 8, 5, 5, 2), count.reshape(21, 8, 5)


def _network(rng, H, L):
    """trunk weights N(0, 9 / fan_in), head weights N(0, 1 / fan_in), biases N(0, 1), rounded to float32: [(W, b)] of the hidden
    layers, then cells, pieces, value"""
    dims = [(H, 1684, 3.0)] + [(H, H, 3.0)] * (L - 1) + [(400, H, 1.0), (21, H, 1.0), (4, H, 1.0)]
    return [((rng.standard_normal(d[:2]) * d[2] / np.sqrt(d[1])).astype(np.float32), rng.standard_normal(d[0]).astype(np.float32)) for d in dims]


def _pack(bb, layers):
    dev = [(torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)) for W, b in layers]
    return bb.net_pack(dev[:-3], dev[-3], dev[-2], dev[-1])


def _features(board, pieces):
    """the contract's feature map: the four owner planes, then the inventories"""
    board = board.reshape(len(board), 400)
    return np.concatenate([board == j for j in range(4)] + [pieces.reshape(len(board), 84) != 0], axis=1)


def _forward(layers, board, pieces):
    """the network in float64 numpy -> the map q [B, 400], the piece terms r [B, 21], v [B, 4]"""
    x = _features(board, pieces).astype(np.float64)
    for W, b in layers[:-3]:
        x = np.maximum(x @ W.astype(np.float64).T + b, 0)
    return [x @ W.astype(np.float64).T + b for W, b in layers[-3:]]


def _outputs(q, r, v, cand, n_cand, mover, pending):
    """the header's candidate logits and integer outputs from the heads' results -> (prior, value, logit with -inf beyond K)"""
    B, W = cand.shape
    cells, count = _offsets()
    a = np.clip(cand.astype(np.int64), 0, IDS - 1)
    piece, anchor, orient, shift = a // 16000, (a // 40) % 400, (a // 5) % 8, a % 5
    n = np.where((cand >= 0) & (cand < IDS), count[piece, orient, shift], 0)        # 0: the pass, a bad id, a shift without a cell
    off = cells[piece, orient, shift]                                               # [B, W, 5, 2]
    X, Y = (anchor % 20)[..., None] + off[..., 0], (anchor // 20)[..., None] + off[..., 1]
    on = (np.arange(5) < n[..., None]) & (X >= 0) & (X < 20) & (Y >= 0) & (Y < 20)  # no wrap-around: a cell off the board adds nothing
    m = (mover.astype(np.int64) & 3)[:, None, None]
    i = np.choose(m, [Y, X, 19 - Y, 19 - X], mode="clip")
    j = np.choose(m, [X, 19 - Y, 19 - X, Y], mode="clip")
    rows = np.arange(B)[:, None, None]
    logit = np.where(n > 0, r[np.arange(B)[:, None], piece], 0) + np.where(on, q[rows, np.clip(20 * i + j, 0, 399)], 0).sum(axis=2)
    K = np.clip(n_cand, 0, W)
    logit = np.where(np.arange(W) < K[:, None], logit, -np.inf)
    with np.errstate(all="ignore"):
        prior = np.round(65535.0 * np.exp(logit - logit.max(axis=1, keepdims=True)))
        value = np.round(65536.0 / (1.0 + np.exp(-v))).astype(np.int64)
    prior = np.where(np.isnan(prior), 0, prior).astype(np.int64)                    # K = 0: a row of -inf
    live = (pending != 0)[:, None]
    return np.where(live, prior, 0), np.where(live, value, 0), logit


def _reference(layers, leaves, pending):
    board, pieces, cand, n_cand, mover = leaves
    return _outputs(*_forward(layers, board, pieces), cand, n_cand, mover, pending)


def _compare(prior, value, want, pending, what):
    """the checks on the rows of a call"""
    want_prior, want_value, logit = want
    prior = prior.view(np.uint16).astype(np.int64)
    live = pending != 0
    assert (prior[~live] == 0).all() and (value[~live] == 0).all(), what
    assert (prior[np.isinf(logit)] == 0).all(), what                              # the slots from K on
    assert (value >= 0).all() and (value <= 65536).all(), what
    some = live & ~np.isinf(logit).all(axis=1)
    assert (prior[some].max(axis=1) == 65535).all(), what
    assert (prior[some, logit[some].argmax(axis=1)] >= 65535 - TOL).all(), what
    dp, dv = int(np.abs(prior - want_prior).max()), int(np.abs(value.astype(np.int64) - want_value).max())
    print("%s: largest deviation prior %d, value %d" % (what, dp, dv))
    assert dp <= TOL and dv <= TOL, (what, dp, dv)


@functools.lru_cache(maxsize=None)
def _case(shape, B):
    """the inputs of a case and the reference's outputs, computed once"""
    H, L, W = SHAPES[shape]
    rng = np.random.default_rng(1000 * shape + B)
    layers = _network(rng, H, L)
    board = rng.integers(-2, 5, size=(B, 20, 20)).astype(np.int8)                  # -2 and 4 set no feature
    pieces = rng.choice(np.array([0, 1, 7], np.uint8), size=(B, 4, 21))
    mover = (np.arange(B) % 4 + 4 * rng.integers(-1, 2, size=B)).astype(np.int8)   # all four movers, high bits set
    n_cand = rng.integers(0, W + 1, size=B).astype(np.int32)
    n_cand[rng.random(B) < 0.1] = W + 3                                            # clamped
    n_cand[0] = W
    count = _offsets()[1]
    piece, orient = rng.integers(0, 21, size=(B, W)), rng.integers(0, 8, size=(B, W))
    shift = rng.integers(0, 5, size=(B, W)) % count[piece, orient, 0]              # a cell of the piece; the anchor anywhere: cells fall off the board
    cand = (((piece * 400 + rng.integers(0, 400, size=(B, W))) * 8 + orient) * 5 + shift).astype(np.int32)
    odd = np.array([-1, -2, IDS, 3], np.int32)                                      # 3: the monomino's shift 3
    cand = np.where(rng.random((B, W)) < 0.1, rng.choice(odd, size=(B, W)), cand)
    pending = (rng.random(B) >= 0.25).astype(np.uint8)
    pending[0] = 1
    if (shape, B) == (1, 17):
        pending = None                                                            # the one case with pending = NULL
    leaves = (board, pieces, cand, n_cand, mover)
    return layers, leaves, pending, _reference(layers, leaves, np.ones(B, np.uint8) if pending is None else pending)


@pytest.mark.parametrize("shape, B", CASES, ids=["h%d_l%d_w%d_b%d" % (SHAPES[s] + (B,)) for s, B in CASES])
def test_net_eval_against_float64(shape, B):
    H, L, W = SHAPES[shape]
    layers, leaves, pending, want = _case(shape, B)
    bb = BlokusBatch(1, device=DEV)
    net = _pack(bb, layers)
    prior = torch.full((B + 3, W), -21931, dtype=torch.int16, device=DEV)
    value = torch.full((B + 3, 4), -77, dtype=torch.int32, device=DEV)
    bb.net_eval(net, *[torch.from_numpy(a).to(DEV) for a in leaves], None if pending is None else torch.from_numpy(pending).to(DEV),
                out=(prior[:B], value[:B]))
    prior, value = _np(prior), _np(value)
    assert (prior[B:] == -21931).all() and (value[B:] == -77).all()               # nothing behind row B is touched
    _compare(prior[:B], value[:B], want, np.ones(B, np.uint8) if pending is None else pending, (shape, B))


def _search(B=32, seed=5):
    bb = BlokusBatch(B, device=DEV)                              # (reset positions)
    layers = _network(np.random.default_rng(seed), 128, 2)
    return bb, layers, _pack(bb, layers)


def test_inside_a_search():
    bb, layers, net = _search()
    S, W, leaves = 6, 8, None
    bb.puct_begin(S, W)
    for s in range(S):
        leaves = bb.puct_select(out=leaves)
        prior, value = bb.net_eval(net, leaves)
        pending = _np(leaves["pending"])
        assert pending.any()
        got = [_np(leaves[key]) for key in ("board", "pieces", "cand", "n_cand", "mover")]
        _compare(_np(prior), _np(value), _reference(layers, got, pending), pending, ("search", s))
        bb.puct_backup(prior, value)
    root = {key: _np(t) for key, t in bb.puct_root().items()}
    assert (root["sims"] == S).all()
    again = bb.puct(net.evaluator(), S, W)
    assert all(np.array_equal(_np(again[key]), root[key]) for key in root)


def test_graph_replays_advance_the_search():
    bb, layers, net = _search()
    W = 8
    want = {key: _np(t) for key, t in bb.puct(net.evaluator(), 2, W).items()}     # the eager run: two simulations
    bb.puct_begin(2, W)
    leaves = bb.puct_select()
    out = bb.net_eval(net, leaves)

    def simulation():
        bb.puct_select(out=leaves)
        bb.puct_backup(*bb.net_eval(net, leaves, out=out))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on a side stream, as torch.cuda.graph wants
        simulation()
    torch.cuda.current_stream().wait_stream(side)
    bb.puct_begin(2, W)                                          # the warm-up was a simulation: start again
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        simulation()
    bb.puct_begin(2, W)                                          # (a capture runs nothing)
    for done in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        assert (_np(bb.puct_root()["sims"]) == done).all()
    got = bb.puct_root()
    assert all(np.array_equal(_np(got[key]), want[key]) for key in want)
