"""The read-only Tron evaluators on the GPU under quarter turns of the board: crl_tron_territory (and territory_action),
crl_tron_sample_avoid, crl_tron_sample_territory, crl_tron_playout, crl_tron_mcts, crl_tron_mcts_territory, and crl_tron_step
without reset.  Their contract is written in relative actions, player indices and draws keyed by (game, counter, player), so
it is exactly equivariant under the turn of tests/tron_rotate.py (held against the restatements and the oracle in
tests/test_tron_rotate_host.py): every output on the turned state must be bit-identical to the output on the state as it
stands.  The kernels are not symmetric under the turn -- a board row is a lane or a word and a column is a bit, vertical
neighbours come by wave shifts and horizontal ones by bit shifts under a row mask, rows are cut out of the flat bitboard in
the middle of a dword -- so a wrong mask, a row edge off by one, a shift leaking across the 32 / 33 edge or a wrong last lane
at 64 breaks the equality.  The GPU is compared with itself, so the batches (64 .. 130 positions: several waves and a ragged
tail), the simulation counts and the board widths are the ones the restatement tests cannot afford.

Widths: 5 (59 idle lanes), 19 and 21 (rows start in the middle of a dword), 31 | 32 | 33, 40, 63 | 64; 65 and 100 for the
calls that have an LDS kernel above 64, 70 for the playout search (which takes boards up to 89).  Every player count 1 .. 8
occurs on both sides of the 32 / 33 edge.  The start layout is not assumed to be symmetric under the turn, so the step is
tested without reset and the rollout entries not at all."""
import functools

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, np_of as _np, tron_put, tron_state
from tests.tron_rotate import rotate

pytestmark = pytest.mark.gpu

CASES = [(5, 1), (5, 2), (19, 3), (19, 4), (21, 5), (31, 6), (32, 7), (32, 8),
         (33, 1), (33, 2), (40, 3), (40, 4), (63, 5), (63, 6), (64, 7), (64, 8)]
WIDE = [(65, 3), (100, 5)]                     # territory, the scripted agents, playout: the LDS kernels
MCTS_WIDE = [(70, 2)]                          # the playout search alone takes 65 .. 89
_ids = lambda cases: ["%dx%dp%d" % (n, n, p) for n, p in cases]
cases = pytest.mark.parametrize("N,P", CASES, ids=_ids(CASES))
cases_and_wide = pytest.mark.parametrize("N,P", CASES + WIDE, ids=_ids(CASES + WIDE))
agents = pytest.mark.parametrize("agent", ["random", "avoid"])
FIRST_ENV_ID = (1 << 32) + 77
TURNS = (1, 2, 3)


def test_cases_cover_every_player_count_on_both_sides_of_32():
    assert {P for N, P in CASES if N <= 32} == {P for N, P in CASES if N > 32} == set(range(1, 9))
    assert {N for N, P in CASES} == {5, 19, 21, 31, 32, 33, 40, 63, 64}


@functools.lru_cache(maxsize=None)
def _positions(N, P):
    """(stepper, state, seat, tcount): 64 .. 130 positions from the GPU's own play, read back once -- the first half from
    random play with auto-reset (sparse boards at different steps), the second half from avoid play on top of it (boards from
    the start layout to nearly full); a few players killed by hand, one finished game, a dead seat and two seats out of range;
    counters that are small, about to wrap and random.  The stepper is shared by the tests of a shape: each uploads what it
    runs on."""
    from colosseumrl_amd.batched import TronBatch
    B = 64 + (N * 7 + P * 3) % 67
    rng = np.random.default_rng(N * 100 + P)
    tb = TronBatch(N, P, B, device=DEV, first_env_id=FIRST_ENV_ID)
    if P == 1:      # every step of a one-player game is terminal, so play with auto-reset never leaves the start layout:
        def play(steps):                                                          # avoid play step by step, no reset
            for _ in range(steps):
                tb.step(tb.sample_avoid(N, 0.1))
        play(4)
        sparse = tron_state(tb)
        play(N)
        full = tron_state(tb)
    else:
        tb.rollout(int(rng.integers(3, 2 * N)), seed=N + P)
        sparse = tron_state(tb)
        tb.rollout_avoid(N * N // (2 * P) + N, seed=N + P, noise=0.1)
        full = tron_state(tb)
    half = B // 2
    board = np.concatenate([sparse[0][:half], full[0][half:]], axis=0)
    heads, dirs, deaths = (np.concatenate([s[:, :half], f[:, half:]], axis=1) for s, f in zip(sparse[1:], full[1:]))
    if P >= 2:
        for b in rng.choice(B - 8, size=B // 8, replace=False):                 # a player killed by hand
            p = int(rng.integers(0, P))
            deaths[p, b] = deaths[p, b] or p + 1
        deaths[:, B - 3] = np.arange(P) + 1                                       # a finished game: one player alive
        deaths[P - 1, B - 3] = 0
    live = deaths == 0
    seat = np.array([rng.choice(np.flatnonzero(live[:, b])) if live[:, b].any() else 0 for b in range(B)], np.int8)
    deaths[seat[B - 2], B - 2] = seat[B - 2] + 1                                  # the seat is dead
    seat[B - 4], seat[B - 5] = P, -1                                              # seats out of range
    tcount = rng.integers(0, 2 ** 32, size=B, dtype=np.uint64).astype(np.uint32)
    tcount[:4] = np.array([3, 7, 8, 2 ** 32 - 3], np.uint64).astype(np.uint32)
    assert (board[np.arange(B)[None, :], heads.astype(np.int64)] == np.arange(1, P + 1)[:, None]).all()
    fill = (board != 0).sum(axis=1)
    assert fill.max() >= 2 * fill.min() and fill.max() > 3 * P                    # the fill levels differ; mid-game boards
    return tb, (board, heads, dirs, deaths), seat, tcount


def _upload(tb, state, tcount):
    tron_put(tb, *state)
    tb.tcount.copy_(torch.from_numpy(tcount.view(np.int32)))


def _under_turns(N, P, run):
    """{k: run(stepper)} for the state as it stands (k = 0) and after 1, 2, 3 quarter turns; every turned state differs from
    the state as it stands.  `run` returns a dict of tensors of its own (not views of the stepper's buffers)."""
    tb, state, seat, tcount = _positions(N, P)
    out = {}
    for k in (0,) + TURNS:
        turned = rotate(N, *state, k=k)
        assert k == 0 or not np.array_equal(turned[0], state[0])
        _upload(tb, turned, tcount)
        out[k] = run(tb)
    return out


def _assert_same(out):
    for k in TURNS:
        assert out[k].keys() == out[0].keys()
        for name in out[0]:
            a, b = out[0][name], out[k][name]
            if not torch.equal(a, b):
                rows = torch.nonzero((a != b).reshape(a.shape[0], -1).any(dim=1)).flatten()[:8].tolist()
                raise AssertionError("%s differs after %d quarter turns, first rows %s" % (name, k, rows))


def _seat_t(N, P):
    return torch.from_numpy(_positions(N, P)[2]).to(DEV)


# ------------------------------------------------------------------ 1. Voronoi territory and the territory-greedy action
@cases_and_wide
def test_territory(N, P):
    """nobody forced; the three candidates with mixed seats (out of range and dead ones among them) and padding: area and
    info; territory_action for the seats"""
    tb, state, seat, _ = _positions(N, P)
    B = tb.B
    rng = np.random.default_rng(N + P)
    mixed = torch.from_numpy(rng.integers(-1, P + 1, size=B).astype(np.int8)).to(DEV)
    cand = torch.from_numpy(rng.integers(-1, 4, size=(B, 5)).astype(np.int32)).to(DEV)
    seat_t = torch.from_numpy(np.clip(seat, 0, P - 1)).to(DEV)

    def run(tb):
        o0, o1 = tb.territory(), tb.territory(cand, mixed)
        return {"area": o0["area"], "info": o0["info"], "area_cand": o1["area"], "info_cand": o1["info"],
                "action": tb.territory_action(seat_t), "action_seat0": tb.territory_action()}

    out = _under_turns(N, P, run)
    _assert_same(out)
    assert int((out[0]["area"] > 0).sum()) > B // 2 and int((out[0]["area_cand"] > 0).sum()) > 0
    info = out[0]["info_cand"]
    assert bool((info == 0).any()) and bool((info == 1).any())                   # skipped rows and evaluated ones
    assert len(torch.unique(out[0]["action"])) >= 3                               # (of -1, 0, 1, 2)


# ------------------------------------------------------------------ 2. the scripted agents
@cases_and_wide
def test_scripted_agents(N, P):
    """sample_avoid and sample_territory for all players at noise 0.1 (the counters are not advanced)"""
    def run(tb):
        return {"avoid": tb.sample_avoid(21, 0.1, advance=False), "territory": tb.sample_territory(21, 0.1, advance=False)}

    out = _under_turns(N, P, run)
    _assert_same(out)
    for name in ("avoid", "territory"):
        assert bool((out[0][name] != 0).any()), name             # (somebody turns)


# ------------------------------------------------------------------ 3. playouts
@cases_and_wide
def test_playout(N, P):
    """both agents, both stop rules, capped and uncapped, forced candidates (mixed, with padding) and none: all four outputs.
    Avoid playouts on the boards above 40x40 are capped (an avoid game there lasts hundreds of steps)."""
    tb, state, seat, _ = _positions(N, P)
    seat_t = _seat_t(N, P)
    cand = torch.from_numpy(np.random.default_rng(N * P).integers(-1, 4, size=(tb.B, 4)).astype(np.int32)).to(DEV)
    cap = 0 if N <= 40 else 24
    runs = [("random", "end", 0, cand), ("random", "seat_done", 6, None), ("avoid", "end", cap, cand), ("avoid", "seat_done", cap, None),
            ("avoid", "end", 5, None)]

    def run(tb):
        got = {}
        for i, (agent, until, max_steps, c) in enumerate(runs):
            o = tb.playout(8, c, 31 + i, agent=agent, noise=0.1, seat=seat_t, until=until, max_steps=max_steps)
            got.update({"%s_%d" % (key, i): o[key] for key in ("wins", "played", "len_sum", "ret_sum")})
        return got

    out = _under_turns(N, P, run)
    _assert_same(out)
    for i in range(len(runs)):
        played, len_sum = out[0]["played_%d" % i], out[0]["len_sum_%d" % i]
        assert int((played > 0).sum()) > tb.B // 2 and bool((played == 0).any())
        assert P == 1 or int(len_sum.sum()) > int(played.sum())                  # (playouts of more than one step)
    assert P == 1 or int(out[0]["wins_0"].sum()) > 0


# ------------------------------------------------------------------ 4. the tree searches
def _reached(o, S, B, P):
    """most trees have more than one node; some went past the root's children (an OPEN child was expanded; with one player
    every child is closed) and some have fewer nodes than simulations + 1 (a CLOSED leaf was visited again), seen through
    `nodes` and `visits`"""
    nodes, visits = _np(o["nodes"]), _np(o["visits"])
    played = nodes > 0
    assert (nodes > 1).sum() > B // 2 and (~played).sum() >= 3
    assert (visits[played].sum(axis=1) == S).all() and (visits[~played] == 0).all()
    assert ((nodes > 4).any() or P == 1) and (nodes[played] < S + 1).any()
    assert ((_np(o["best"]) >= 0) == played).all()


@pytest.mark.parametrize("N,P", CASES + MCTS_WIDE, ids=_ids(CASES + MCTS_WIDE))
@agents
def test_mcts(N, P, agent):
    """S = 200 simulations of R = 8 playouts, capped above 21x21"""
    seat_t = _seat_t(N, P)
    S = 200

    def run(tb):
        return dict(tb.mcts(S, 8, seed=5, exploration=1.0, agent=agent, noise=0.1, seat=seat_t, max_steps=0 if N <= 21 else 12))

    out = _under_turns(N, P, run)
    _assert_same(out)
    _reached(out[0], S, _positions(N, P)[0].B, P)
    assert int(out[0]["value"].sum()) > 0


@cases
@agents
def test_mcts_territory(N, P, agent):
    """S = 300 simulations, one flood a leaf"""
    seat_t = _seat_t(N, P)
    S = 300

    def run(tb):
        return dict(tb.mcts_territory(S, seed=5, exploration=1.0, agent=agent, noise=0.1, seat=seat_t))

    out = _under_turns(N, P, run)
    _assert_same(out)
    _reached(out[0], S, _positions(N, P)[0].B, P)
    value, visits = _np(out[0]["value"]), _np(out[0]["visits"])
    assert P == 1 or ((value % 512 != 0) & (visits > 0)).any()                   # (a flooded leaf: closed ones are worth 0 or 2 V)


# ------------------------------------------------------------------ 5. the step, without reset
@cases_and_wide
def test_step_commutes_with_the_turn(N, P):
    """three steps of random actions in a row, no reset: rewards, terminal and winners are equal, and the state afterwards is
    the turned state of the unturned run"""
    tb, state, seat, tcount = _positions(N, P)
    acts = [torch.from_numpy(np.random.default_rng(N * P + t).integers(-1, 2, size=(P, tb.B)).astype(np.int8)).to(DEV)
            for t in range(3)]

    def run(tb):
        got = {}
        for t, act in enumerate(acts):
            rew, term, win = tb.step(act)
            got.update({"rewards_%d" % t: rew.clone(), "terminal_%d" % t: term.clone(), "winners_%d" % t: win.clone()})
            got["state_%d" % t] = tron_state(tb)
        return got

    out = _under_turns(N, P, run)
    states = {k: [out[k].pop("state_%d" % t) for t in range(3)] for k in out}
    _assert_same(out)
    for k in TURNS:
        for t in range(3):
            want = rotate(N, *states[0][t], k=k)
            for name, g, w in zip(("board", "heads", "dirs", "deaths"), states[k][t], want):
                assert np.array_equal(g, w), (name, k, t)
    assert (states[0][2][3] != 0).sum() > (state[3] != 0).sum()                    # (somebody died)
    assert not np.array_equal(states[0][2][0], state[0])
