"""The policy-value MLP of the TicTacToe search in one launch (crl_ttt_net_eval, TTTBatch.net_pack / net_eval) against the same
network in float64 numpy, at every shape where the kernel takes another path and B below a tile, with a ragged second tile,
over many workgroups and past the grid (the grid-stride loop); then inside a search and under a graph.
Tolerance: 4 output units.  The same networks in float32 by torch on the CPU differ from float64 by at most 1 unit at this
weight scale; the margin covers another summation order and the hardware exponential, and any indexing, masking or layout
error moves values by thousands.  Largest deviation measured on an MI355X over every case below: prior 1, value 1."""
import functools

import numpy as np
import pytest
import torch

from colosseumrl_amd.batched import TTTBatch
from tests.gpu_util import DEV, np_of as _np, u32_of

pytestmark = pytest.mark.gpu
TOL = 4
SHAPES = [((3, 3), 3, 2, 16, 1), ((3, 5), 3, 3, 64, 2), ((3, 3, 3), 3, 4, 48, 3), ((5, 5), 4, 3, 256, 2)]     # dims, k, P, H, L
CASES = [(s, B) for s in range(4) for B in (1, 17, 5000)] + [(0, 2048 * 16 + 17)]       # the last: more tiles than the grid holds


def _network(rng, cells, P, C, H, L):
    """weights N(0, 9 / fan_in) and biases N(0, 1), rounded to float32: [(W, b)] of the hidden layers, the policy and the value head"""
    dims = [(H, cells * C)] + [(H, H)] * (L - 1) + [(cells, H), (P, H)]
    return [((rng.standard_normal(d) * 3.0 / np.sqrt(d[1])).astype(np.float32), rng.standard_normal(d[0]).astype(np.float32)) for d in dims]


def _pack(tb, layers, C=None):
    dev = [(torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)) for W, b in layers]
    return tb.net_pack(dev[:-2], dev[-2], dev[-1], C)


def _reference(layers, C, board, valid, pending):
    """float64: (prior, value, the logits with -inf at the cells outside `valid`)"""
    x = (board[:, :, None] == np.arange(C)).reshape(len(board), -1).astype(np.float64)
    for W, b in layers[:-2]:
        x = np.maximum(x @ W.astype(np.float64).T + b, 0.0)
    (Wp, bp), (Wv, bv) = layers[-2:]
    logit, v = x @ Wp.astype(np.float64).T + bp, x @ Wv.astype(np.float64).T + bv
    E = ((valid[:, None] >> np.arange(board.shape[1], dtype=np.uint32)) & 1).astype(bool)
    masked = np.where(E, logit, -np.inf)
    with np.errstate(all="ignore"):
        prior = np.where(E, np.round(65535.0 * np.exp(logit - masked.max(axis=1, keepdims=True))), 0.0)
        value = np.round(65536.0 / (1.0 + np.exp(-v)))
    live = (pending != 0)[:, None]
    return np.where(live, prior, 0).astype(np.int64), np.where(live, value, 0).astype(np.int64), masked


def _compare(prior, value, want, valid, pending, what):
    """the checks of the issue on rows that were evaluated -> the largest deviations"""
    want_prior, want_value, masked = want
    cells = prior.shape[1]
    prior = prior.view(np.uint16).astype(np.int64)
    E = ((valid[:, None] >> np.arange(cells, dtype=np.uint32)) & 1).astype(bool)
    live = pending != 0
    assert (prior[~live] == 0).all() and (value[~live] == 0).all(), what
    assert (prior[~E] == 0).all(), what
    assert (value >= 0).all() and (value <= 65536).all(), what
    ranked = np.sort(masked, axis=1)
    with np.errstate(invalid="ignore"):                                          # (-inf - -inf where no cell is valid: not close)
        close = ranked[:, -1] - ranked[:, -2] <= 1e-5
    decided = live & E.any(axis=1) & ~close
    assert (close & live).sum() < 0.01 * max(len(prior), 100), what
    assert (prior[decided, masked[decided].argmax(axis=1)] == 65535).all(), what
    dp, dv = int(np.abs(prior - want_prior).max()), int(np.abs(value.astype(np.int64) - want_value).max())
    print("%s: largest deviation prior %d, value %d" % (what, dp, dv))
    assert dp <= TOL and dv <= TOL, (what, dp, dv)
    return dp, dv


@functools.lru_cache(maxsize=None)
def _case(shape, B):
    """the inputs of a case and the reference's outputs, computed once"""
    dims, k, P, H, L = SHAPES[shape]
    cells = int(np.prod(dims))
    rng = np.random.default_rng(1000 * shape + B)
    layers = _network(rng, cells, P, P, H, L)
    board = rng.integers(-1, P, size=(B, cells)).astype(np.int8)
    board[rng.random((B, cells)) < 0.05] = P                                      # a value without a feature
    valid = (rng.integers(0, 1 << 32, size=B, dtype=np.uint64) & ((1 << cells) - 1)).astype(np.uint32)    # independent of the board
    single = rng.random(B) < 0.1
    valid[single] = np.uint32(1) << rng.integers(0, cells, size=B).astype(np.uint32)[single]
    valid[rng.random(B) < 0.02] = 0
    pending = (rng.random(B) >= 0.25).astype(np.uint8)
    pending[0] = 1
    if (shape, B) == (1, 17):
        pending = None                                                            # the one case with pending = NULL
    want = _reference(layers, P, board, valid, np.ones(B, np.uint8) if pending is None else pending)
    return layers, board, valid, pending, want


@pytest.mark.parametrize("shape, B", CASES, ids=["%s_h%d_l%d_b%d" % ("x".join(map(str, SHAPES[s][0])), SHAPES[s][3], SHAPES[s][4], B) for s, B in CASES])
def test_net_eval_against_float64(shape, B):
    dims, k, P, H, L = SHAPES[shape]
    layers, board, valid, pending, want = _case(shape, B)
    tb = TTTBatch(dims, k, P, 1, device=DEV)
    net = _pack(tb, layers)
    prior = torch.full((B + 3, tb.n_cells), -21931, dtype=torch.int16, device=DEV)
    value = torch.full((B + 3, P), -77, dtype=torch.int32, device=DEV)
    got = tb.net_eval(net, torch.from_numpy(board).to(DEV), torch.from_numpy(valid.view(np.int32)).to(DEV),
                      None if pending is None else torch.from_numpy(pending).to(DEV), out=(prior[:B], value[:B]))
    prior, value = _np(prior), _np(value)
    assert (prior[B:] == -21931).all() and (value[B:] == -77).all()               # nothing behind row B is touched
    _compare(prior[:B], value[:B], want, valid, np.ones(B, np.uint8) if pending is None else pending, (shape, B))


def _search(B=64, seed=5):
    dims, k, P, H, L = SHAPES[1]
    tb = TTTBatch(dims, k, P, B, device=DEV)
    layers = _network(np.random.default_rng(seed), tb.n_cells, P, P, H, L)
    return tb, layers, _pack(tb, layers)


def test_inside_a_search():
    tb, layers, net = _search()
    S, leaves = 8, None
    tb.puct_begin(S)
    for s in range(S):
        leaves = tb.puct_select(out=leaves)
        prior, value = tb.net_eval(net, leaves)
        board, valid, pending = _np(leaves["board"]), u32_of(leaves["valid"]), _np(leaves["pending"])
        assert pending.any()
        _compare(_np(prior), _np(value), _reference(layers, tb.P, board, valid, pending), valid, pending, ("search", s))
        tb.puct_backup(prior, value)
    root = {key: _np(t) for key, t in tb.puct_root().items()}
    assert (root["sims"] == S).all()
    again = tb.puct(net.evaluator(), S)
    assert all(np.array_equal(_np(again[key]), root[key]) for key in root)


def test_graph_replays_advance_the_search():
    tb, layers, net = _search()
    want = {key: _np(t) for key, t in tb.puct(net.evaluator(), 2).items()}        # the eager run: two simulations
    tb.puct_begin(2)
    leaves = tb.puct_select()
    out = tb.net_eval(net, leaves)

    def simulation():
        tb.puct_select(out=leaves)
        tb.puct_backup(*tb.net_eval(net, leaves, out=out))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on a side stream, as torch.cuda.graph wants
        simulation()
    torch.cuda.current_stream().wait_stream(side)
    tb.puct_begin(2)                                             # the warm-up was a simulation: start again
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        simulation()
    tb.puct_begin(2)                                             # (a capture runs nothing)
    for done in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        assert (_np(tb.puct_root()["sims"]) == done).all()
    got = tb.puct_root()
    assert all(np.array_equal(_np(got[key]), want[key]) for key in want)
