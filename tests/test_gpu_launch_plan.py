"""Launch plans on the GPU: a stepper that rolls out through its bound plan and the C-API entry (what `rollout()` does) against
a twin that calls the rollout entry of the C ABI directly with the same arguments -- state, every statistics tensor and both
result rows bit for bit.  The direct path is held to the oracle by the suites of the three games; this file holds the plan to
the direct path: a wrong or stale argument in a plan (batch, first_env_id, a pointer, the flags, the seed's high word, the
stream) shows as a difference here."""
import pytest
import torch

from colosseumrl_amd import _native
from colosseumrl_amd.batched import _ROLLOUT_KERNEL_FLAGS, BlokusBatch, TronBatch, TTTBatch, _stream

pytestmark = pytest.mark.gpu

FIRST = 2 ** 32 + 3                        # the game ids reach the kernels as 64 bits
SEEDS = (2 ** 32 + 7, 2 ** 64 - 1)         # ... and so does the seed: both Philox key words are in use
STEPS = (1, 5, 20, 37)                     # one step, a short launch, the benchmark's launch, one across a 32-step action refill
LDS_PINS = ("auto", "quad", "qbits", "bits", "bytes", "global", "gquad")
# (N, P) -> the pins that select a kernel of their own there: "pair" needs at most two players, "quad" boards up to 20x20
TRON_SHAPES = {(20, 4): LDS_PINS, (19, 4): LDS_PINS, (7, 2): LDS_PINS + ("pair",),
               (24, 4): ("auto", "qbits", "bits", "bytes", "global", "gquad")}
TRON_STATE = ("board", "heads", "dirs", "deaths")


def _direct_tron(tb, T, seed, kernel="auto"):
    """crl_tron_rollout itself, with the arguments the stepper's plan was bound to"""
    rc = tb._lib.crl_tron_rollout(tb._ctx.handle, tb.B, seed, tb.first_env_id, T, *tb._state(), tb._stats(),
                                  _ROLLOUT_KERNEL_FLAGS[kernel], _stream())
    _native.check(rc, "crl_tron_rollout")


def _same(a, b, state, what):
    torch.cuda.synchronize()
    for k in state:
        assert torch.equal(getattr(a, k), getattr(b, k)), (k, what)
    for k, x, y in zip(a.STATS, a._stat_tensors(), b._stat_tensors()):
        assert torch.equal(x, y), (k, what)


def _tron_pair(N, P, B):
    a, b = (TronBatch(N, P, B, first_env_id=FIRST) for _ in range(2))
    return a, b


def _uses_fast_entry(tb):
    assert tb._launch is _native.fast().rollout_launch and tb._plans


@pytest.mark.parametrize("N,P,kernel", [(N, P, k) for (N, P), pins in TRON_SHAPES.items() for k in pins])
def test_tron_plan_equals_direct_call(N, P, kernel):
    """B = 67: ragged against the 16 games of a quad kernel's wave and the 64 of a workgroup.  The launches follow each other
    on the same state, so every one starts from counters and boards the one before left."""
    B = 67
    a, b = _tron_pair(N, P, B)
    steps = 0
    for seed in SEEDS:
        for T in STEPS:
            a.rollout(T, seed, kernel=kernel)
            _direct_tron(b, T, seed, kernel)
            steps += T
            _same(a, b, TRON_STATE, (seed, T))
    _uses_fast_entry(a)
    assert b._plans is None                                   # the twin never went through a plan
    assert int(a.tcount.sum()) == B * steps and int(a.n_episodes.sum()) > 0
    assert torch.equal(a.results(), b.results()) and torch.equal(a._packed, b._packed)


def test_tron_plan_through_ctypes_equals_direct_call(monkeypatch):
    """CRL_NO_FASTCALL=1: the same plan launched through ctypes"""
    monkeypatch.setenv("CRL_NO_FASTCALL", "1")
    a, b = _tron_pair(20, 4, 67)
    for seed in SEEDS:
        for T in STEPS:
            a.rollout(T, seed)
            _direct_tron(b, T, seed)
    assert a._launch is a._lib.crl_rollout_launch or a._launch.__name__ == "crl_rollout_launch"
    _same(a, b, TRON_STATE, "ctypes")
    assert int(a.tcount.sum()) == 67 * 2 * sum(STEPS)


def test_tron_plan_on_a_side_stream():
    """the launch goes to torch's CURRENT stream at the time of the call, not to one bound with the plan: a rollout on a
    side stream, then a copy on that stream that depends on it"""
    a, b = _tron_pair(20, 4, 67)
    a.rollout(5, SEEDS[0])                                    # binds the plan on the default stream
    _direct_tron(b, 5, SEEDS[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    copies = []
    for tb, go in ((a, lambda: a.rollout(20, SEEDS[1])), (b, lambda: _direct_tron(b, 20, SEEDS[1]))):
        with torch.cuda.stream(side):
            go()
            copies.append((tb.board.clone(), tb.results()))
    side.synchronize()
    _uses_fast_entry(a)
    assert torch.equal(copies[0][0], copies[1][0]) and torch.equal(copies[0][1], copies[1][1])
    assert torch.equal(copies[0][0], a.board) and int(a.tcount.sum()) == 67 * 25
    _same(a, b, TRON_STATE, "side stream")


def test_tron_plan_is_graph_capturable():
    """a launch through the plan records into a HIP graph and replays to what direct eager calls give"""
    a, b = _tron_pair(20, 4, 67)
    for T in (4, 16):                       # warm-up outside capture, as for the rollout entry; the plan is bound here
        a.rollout(T, SEEDS[0])
        _direct_tron(b, T, SEEDS[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.rollout(16, SEEDS[1])
    for _ in range(3):                      # capture itself does not execute: 3 replays == 3 eager launches
        g.replay()
        _direct_tron(b, 16, SEEDS[1])
    _uses_fast_entry(a)
    _same(a, b, TRON_STATE, "graph")
    assert int(a.tcount[0]) == 20 + 3 * 16


def test_tron_plan_splits_a_long_rollout_as_the_entry_does():
    """T = 16384 + 5 on the lane-per-player kernel: one call becomes two launches (16,383 steps at most each)"""
    T = 16384 + 5
    a, b = (TronBatch(7, 4, 16, first_env_id=FIRST) for _ in range(2))
    a.rollout(T, SEEDS[0])
    _direct_tron(b, T, SEEDS[0])
    _uses_fast_entry(a)
    _same(a, b, TRON_STATE, "split")
    assert int(a.tcount[0]) == T and int(a.n_episodes.min()) > 100


def test_ttt_plan_equals_direct_call():
    B, T = 131, 9
    a, b = (TTTBatch((3, 5), 3, 3, B, first_env_id=FIRST) for _ in range(2))
    for seed in SEEDS:
        a.rollout(T, seed)
        _native.check(b._lib.crl_ttt_rollout(b._ctx.handle, B, seed, FIRST, T, *b._state(), b._stats(), _stream()), "crl_ttt_rollout")
        _same(a, b, ("occ", "winner", "to_move"), seed)
    _uses_fast_entry(a)
    assert b._plans is None
    assert int(a.tcount.sum()) == B * 2 * T and int(a.n_episodes.sum()) > 0
    assert torch.equal(a.results(), b.results())


def test_blokus_plan_equals_direct_call():
    B, T = 33, 7
    a, b = (BlokusBatch(B, first_env_id=FIRST) for _ in range(2))
    for seed in SEEDS:
        a.rollout(T, seed)
        _native.check(b._lib.crl_blokus_rollout(b._ctx.handle, B, seed, FIRST, T, *b._state(), b._stats(), _stream()),
                      "crl_blokus_rollout")
        _same(a, b, ("occ", "inv", "score", "round", "to_move"), seed)
    _uses_fast_entry(a)
    assert b._plans is None
    assert int(a.tcount.sum()) == B * 2 * T
    assert torch.equal(a.results(), b.results())


def test_plans_are_unbound_with_the_stepper():
    a = TronBatch(7, 2, 16)
    a.rollout(3, 1)
    a.rollout(3, 1, kernel="gquad")
    assert sorted(a._plans) == [0, _ROLLOUT_KERNEL_FLAGS["gquad"]] and all(a._plans.values())
    a.__del__()
    assert a._plans is None
    a.rollout(2, 1)                                            # (binds afresh)
    torch.cuda.synchronize()
    assert int(a.tcount[0]) == 8


def test_a_new_first_env_id_reaches_the_next_launch():
    """callers set `first_env_id` on a live stepper: the plan bound with the old id must not outlive it"""
    a, b = (TronBatch(7, 2, 67) for _ in range(2))
    a.rollout(20, SEEDS[0])
    _direct_tron(b, 20, SEEDS[0])
    a.first_env_id = b.first_env_id = FIRST
    assert a._plans is None
    a.rollout(20, SEEDS[0])
    _direct_tron(b, 20, SEEDS[0])
    _same(a, b, TRON_STATE, "first_env_id")
    c = TronBatch(7, 2, 67)                                    # ... and the id matters: game ids 0.. give other games
    c.rollout(20, SEEDS[0])
    c.rollout(20, SEEDS[0])
    torch.cuda.synchronize()
    assert not torch.equal(a.board, c.board)
