"""The policy-value MLP of the Tron search in one launch (crl_tron_net_eval, TronBatch.net_pack / net_eval) against the same
network in float64 numpy, at the shapes where the kernel takes another path (plane edges inside a k tile, fewer output tiles
than waves, one to four tiles a wave) and B below a tile, with a ragged second tile, over many workgroups and past the grid
(the grid-stride loop); then inside a search and under a graph.
Tolerance: 4 output units.  The same networks in float32 by torch on the CPU differ from float64 by at most 1 unit (prior
and value) on every case below; the margin covers another summation order and the hardware exponential, and any indexing, masking
or layout error moves values by thousands.  Largest deviation measured on an MI355X over every case below: prior 1, value 1."""
import functools

import numpy as np
import pytest
import torch

from colosseumrl_amd.batched import TronBatch
from tests.gpu_util import DEV, np_of as _np

pytestmark = pytest.mark.gpu
TOL = 4
SHAPES = [(5, 2, 16, 1), (6, 3, 48, 3), (11, 4, 128, 2), (20, 4, 256, 2)]               # N, P, H, L
BLOCK_CAP = 1024                           # the kernel's workgroups per launch (TN_MAX_BLOCKS), 16 leaves each and trip
CASES = [(s, B) for s in range(4) for B in (1, 17, 5000)] + [(0, BLOCK_CAP * 16 + 17)]  # the last: more tiles than the grid holds


def _network(rng, N, H, L):
    """weights N(0, 9 / fan_in) and biases N(0, 1), rounded to float32: [(W, b)] of the hidden layers, the policy and the value head"""
    dims = [(H, 4 * N * N + 4)] + [(H, H)] * (L - 1) + [(3, H), (1, H)]
    return [((rng.standard_normal(d) * 3.0 / np.sqrt(d[1])).astype(np.float32), rng.standard_normal(d[0]).astype(np.float32)) for d in dims]


def _pack(tb, layers):
    dev = [(torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)) for W, b in layers]
    return tb.net_pack(dev[:-2], dev[-2], dev[-1])


def _features(N, board, heads, dirs):
    """the contract's feature map: planes empty / own / other / head, then the facing"""
    cells = np.arange(N * N)
    head = cells == np.clip(heads[0].astype(np.int64), 0, N * N - 1)[:, None]
    facing = (dirs[0].astype(np.int64) & 3)[:, None] == np.arange(4)
    return np.concatenate([board == 0, board == 1, board > 1, head, facing], axis=1)


def _reference(layers, N, board, heads, dirs, pending):
    """the network in float64 numpy -> (prior, value) as integers with zeros on the rows that are not pending, the logits"""
    x = _features(N, board, heads, dirs).astype(np.float64)
    for W, b in layers[:-2]:
        x = np.maximum(x @ W.astype(np.float64).T + b, 0)
    (Wp, bp), (Wv, bv) = layers[-2:]
    logit, v = x @ Wp.astype(np.float64).T + bp, (x @ Wv.astype(np.float64).T + bv)[:, 0]
    with np.errstate(all="ignore"):
        prior = np.round(65535.0 * np.exp(logit - logit.max(axis=1, keepdims=True))).astype(np.int64)
        value = np.round(65536.0 / (1.0 + np.exp(-v))).astype(np.int64)
    live = pending != 0
    return np.where(live[:, None], prior, 0), np.where(live, value, 0), logit


def _compare(prior, value, want, pending, what):
    """the checks on rows that were evaluated"""
    want_prior, want_value, logit = want
    prior = prior.view(np.uint16).astype(np.int64)
    live = pending != 0
    assert (prior[~live] == 0).all() and (value[~live] == 0).all(), what
    assert (value >= 0).all() and (value <= 65536).all(), what
    assert (prior[live].max(axis=1) == 65535).all(), what
    assert (prior[live, logit[live].argmax(axis=1)] >= 65535 - TOL).all(), what
    dp, dv = int(np.abs(prior - want_prior).max()), int(np.abs(value.astype(np.int64) - want_value).max())
    print("%s: largest deviation prior %d, value %d" % (what, dp, dv))
    assert dp <= TOL and dv <= TOL, (what, dp, dv)


@functools.lru_cache(maxsize=None)
def _case(shape, B):
    """the inputs of a case and the reference's outputs, computed once"""
    N, P, H, L = SHAPES[shape]
    rng = np.random.default_rng(1000 * shape + B)
    layers = _network(rng, N, H, L)
    board = rng.integers(-1, P + 2, size=(B, N * N)).astype(np.int8)             # a negative value and one above P included
    heads = rng.integers(0, N * N, size=(P, B)).astype(np.int16)
    heads[:, rng.random(B) < 0.1] = -7
    heads[:, rng.random(B) < 0.1] = N * N + 5
    dirs = rng.integers(-128, 128, size=(P, B)).astype(np.int8)                   # high bits set
    pending = (rng.random(B) >= 0.25).astype(np.uint8)
    pending[0] = 1
    if (shape, B) == (1, 17):
        pending = None                                                            # the one case with pending = NULL
    want = _reference(layers, N, board, heads, dirs, np.ones(B, np.uint8) if pending is None else pending)
    return layers, board, heads, dirs, pending, want


@pytest.mark.parametrize("shape, B", CASES, ids=["n%d_p%d_h%d_l%d_b%d" % (SHAPES[s] + (B,)) for s, B in CASES])
def test_net_eval_against_float64(shape, B):
    N, P, H, L = SHAPES[shape]
    layers, board, heads, dirs, pending, want = _case(shape, B)
    tb = TronBatch(N, P, 1, device=DEV)
    net = _pack(tb, layers)
    prior = torch.full((B + 3, 3), -21931, dtype=torch.int16, device=DEV)
    value = torch.full((B + 3,), -77, dtype=torch.int32, device=DEV)
    tb.net_eval(net, torch.from_numpy(board).to(DEV), torch.from_numpy(heads).to(DEV), torch.from_numpy(dirs).to(DEV),
                None if pending is None else torch.from_numpy(pending).to(DEV), out=(prior[:B], value[:B]))
    prior, value = _np(prior), _np(value)
    assert (prior[B:] == -21931).all() and (value[B:] == -77).all()               # nothing behind row B is touched
    _compare(prior[:B], value[:B], want, np.ones(B, np.uint8) if pending is None else pending, (shape, B))


def _search(B=64, seed=5):
    N, P, H, L = SHAPES[2]
    tb = TronBatch(N, P, B, device=DEV)                           # (reset positions)
    layers = _network(np.random.default_rng(seed), N, H, L)
    return tb, layers, _pack(tb, layers)


def test_inside_a_search():
    tb, layers, net = _search()
    S, leaves = 8, None
    tb.puct_begin(S)
    for s in range(S):
        leaves = tb.puct_select(out=leaves)
        prior, value = tb.net_eval(net, leaves)
        pending = _np(leaves["pending"])
        assert pending.any()
        want = _reference(layers, tb.N, _np(leaves["obs_board"]), _np(leaves["obs_heads"]), _np(leaves["obs_dirs"]), pending)
        _compare(_np(prior), _np(value), want, pending, ("search", s))
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
