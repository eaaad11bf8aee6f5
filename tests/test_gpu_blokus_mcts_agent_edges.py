"""The copy of the search that the Blokus search agent holds (blokus_mcts_agent_kernel), at the edges of
tests/blokus_mcts_cases.py: on every case with a widening root sample_mcts(noise = 0, advance = False) is `best` of
crl_blokus_mcts on the GPU itself -- which tests/test_gpu_blokus_mcts_edges.py holds to the restatement --; for a case with
three trees per workgroup and for the capped rows with a workgroup per game rollout_mcts(1) and step_single(opponent =
"mcts") are sample_mcts followed by step; and the chain and an S = S_max case are also compared with the agent's own
restatement (tests/blokus_mcts_agent_ref.py).

The agent's one output is the move, so these tests see a fault of its copy only where it changes `best`: of the scratch
mutations of the two texts, the one-trip backup and the probe that wraps to rank 1 fail tests/test_gpu_blokus_mcts_edges.py
in crl_blokus_mcts and pass here in the agent's copy (docs/history.md has the table).

The restatement's share: 1.7 s for the chain, 1.6 s for the S_max row; everything else runs on the GPU alone.  Beside an
MI355X the slowest test took 2.2 s (chain_R1: the first launch) and the 29 tests of the file 5.3 s."""
import functools

import numpy as np
import pytest

from tests import blokus_mcts_agent_ref as A
from tests import blokus_mcts_cases as C
from tests import test_gpu_blokus_mcts_edges as E
from tests.blokus_ref import blokus_one, blokus_rank_of
from tests.gpu_util import DEV, blokus_batch, np_of, u32_of

pytestmark = pytest.mark.gpu

STATE = ("occ", "inv", "score", "round", "to_move")
WIDENING = [c.name for c in C.CASES.values() if not c.cand]
COMPOSED = ["trees_S416", "capped_R5_c256", "capped_R5_c65535"]


def _kw(c):
    return dict(simulations=c.S, playouts=c.R, width=c.W, exploration=c.cexp / 256.0, noise=0.0)


def _batch(name):
    r = C.rows(C.CASES[name].rows)
    return blokus_batch(r.state, r.first_env_id, r.tcount)


@functools.lru_cache(maxsize=None)
def _sample(name):
    """(actions of sample_mcts(noise = 0, advance = False) on the rows of case `name`, the state was only read)"""
    bb = _batch(name)
    before = [u32_of(getattr(bb, k)).copy() for k in E.STATE]
    act = np_of(bb.sample_mcts(seed=C.SEED, advance=False, **_kw(C.CASES[name]))).copy()
    return act, all(np.array_equal(a, u32_of(getattr(bb, k))) for a, k in zip(before, E.STATE))


def test_the_cases():
    """every case but the two with candidates (the agent has no candidate root); the composed ones are what they are for"""
    assert len(WIDENING) == len(C.CASES) - 2 == 20
    assert C.trees_per_workgroup(C.CASES["trees_S416"].S) == 3 and C.CASES["trees_S416"].R == 1
    assert all(C.CASES[n].kind == "capped" and C.CASES[n].R == 5 and C.CASES[n].S == 120 for n in COMPOSED[1:])


@pytest.mark.parametrize("name", WIDENING)
def test_sample_is_best(name):
    act, read_only = _sample(name)
    best = E._gpu(name)["best"]
    print(act.tolist(), best.tolist())
    assert np.array_equal(act, best) and read_only
    assert ((act >= 0) | (act == -1)).all()


@pytest.mark.parametrize("name,b", [("chain_R1", 0), ("smax_R4_c65535", 0)])
def test_sample_against_the_restatement(name, b):
    c, r = C.CASES[name], C.rows(C.CASES[name].rows)
    kinds = []
    want = A.agent_action(blokus_one(r.state, b), int(r.tcount[b]), (r.first_env_id + b) & 0xFFFFFFFF, C.SEED, c.W, c.S, c.R, c.cexp,
                          0.0, kinds=kinds)
    assert kinds == ["searched"] and _sample(name)[0][b] == want >= 0


@pytest.mark.parametrize("name", COMPOSED)
def test_rollout_one_step_is_sample_then_step(name):
    """rollout_mcts(1) == sample_mcts; step with auto-reset: state, counters and results rows (the composition's rows are
    counted here; the final scores come from a twin that plays the ply without the reset), the composition of
    test_rollout_is_sample_then_step in tests/test_gpu_blokus_mcts_agent.py"""
    import torch
    kw = _kw(C.CASES[name])
    a, b, probe = _batch(name), _batch(name), _batch(name)
    B = a.B
    a.rollout_mcts(1, seed=C.SEED, **kw)
    act = b.sample_mcts(seed=C.SEED, **kw)
    assert np.array_equal(np_of(act), _sample(name)[0])
    probe.step(act, auto_reset=False)
    final = np_of(probe.score).astype(np.int64)
    _, term, ws = b.step(act, auto_reset=True)
    term, ws = np_of(term).astype(bool), np_of(ws).astype(np.int64)
    rows = np.zeros((B, 10), np.int64)
    rows[term, 0] = 1
    rows[term, 1] = 1
    for q in range(4):
        rows[term, 2 + q] = (ws[term] >> q) & 1
        rows[term, 6 + q] = final[term, q]
    for k in STATE + ("tcount",):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(np_of(a.results()).astype(np.int64), rows)
    assert np.array_equal(np_of(a.tstep).astype(np.int64), np.where(term, 0, 1))
    assert np.array_equal(np_of(a.results_from_columns()), np_of(a.results()))
    assert term.sum() >= (B if C.CASES[name].kind == "capped" else 1)         # (a capped row's every action ends the game)


@pytest.mark.parametrize("name", COMPOSED)
def test_step_single_is_sample_then_step(name):
    """step_single(learner_action = None, opponent = "mcts") for the learner in the seat behind the mover's == while it is not
    the learner's turn (six plies at most): sample_mcts; step with auto-reset; the counter advances -- a game that ends on
    the way restarts, and the searches go on from the empty board until the learner is to move"""
    import torch
    kw = _kw(C.CASES[name])
    a, b, probe = _batch(name), _batch(name), _batch(name)
    B = a.B
    seat = (np_of(a.to_move) + 1) & 3
    seat_t = torch.from_numpy(seat.astype(np.int8)).to(DEV)
    o = a.step_single(seat_t, None, C.SEED, opponent="mcts", **kw)
    live = torch.ones(B, dtype=torch.bool, device=DEV)
    done, winners, reward = np.zeros(B, np.uint8), np.zeros(B, np.uint8), np.zeros(B, np.int8)
    plies = 0
    for _ in range(6):
        live &= (b.to_move & 3) != seat_t.to(torch.int32)
        if not bool(live.any()):
            break
        act = b.sample_mcts(seed=C.SEED, advance=False, **kw)
        saved = {k: getattr(b, k).clone() for k in STATE}
        for k in STATE:
            getattr(probe, k).copy_(saved[k])
        probe.step(act, auto_reset=False)
        final = np_of(probe.score)
        _, term, ws = b.step(act, auto_reset=True)
        for k in STATE:                                         # a game that is not played stays as it was
            t = getattr(b, k)
            t.copy_(torch.where(live.view([B] + [1] * (t.dim() - 1)), t, saved[k]))
        b.tcount.add_(live.to(torch.int32))
        ended = np_of(live) & np_of(term).astype(bool)
        for g in np.flatnonzero(ended):
            done[g], winners[g], reward[g] = 1, np_of(ws)[g], blokus_rank_of(final[g], int(seat[g]))
        plies += int(live.sum())
    for k in STATE + ("tcount",):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert ((np_of(a.to_move) & 3) == seat).all() and plies >= B
    assert np.array_equal(np_of(o["done"]), done) and np.array_equal(np_of(o["winners"]), winners)
    assert np.array_equal(np_of(o["reward"]), reward)
    obs = b.observe(seat_t)
    assert torch.equal(o["n_valid"], b.valid(seat_t))
    for k in ("board", "pieces", "score"):
        assert torch.equal(o[k], obs[k]), k
    assert done.sum() >= (B if C.CASES[name].kind == "capped" else 1)
