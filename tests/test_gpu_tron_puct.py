"""The Tron search valued by the caller's network on the GPU (crl_tron_puct_*, TronBatch.puct_*): the `root` outputs and the
`select` outputs of EVERY simulation bit for bit against the plain-Python restatement of the header's contract
(tests/tron_puct_ref.py), the test evaluator applied on the host between `select` and `backup` -- the shapes of
tests/tron_puct_cases.py (every player count from 1 to 8), positions from the start layout to walled-up boards with skipped ones
among them, B of 1, 5 and 130, the edge rows, a path deeper than 64 nodes, boards below 16 cells, output rows at odd byte
offsets, the boards on either side of every change of `select`'s workgroup shape up to 181x181, trees of 4,095 simulations,
the rows that meet every crash kind of the step --, the game state untouched, the batch stepped while a search is open, the
pair captured into a graph, the wrappers, and a `puct_action` learner valued by territory next to the avoid learner."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import tron_puct_cases as CASES
from tests import tron_puct_ref as R
from tests.gpu_util import DEV, first_episodes, np_of as _np, tron_device_evaluator as _device_evaluator, tron_put, tron_state, u32_of

pytestmark = pytest.mark.gpu
ROOT_KEYS = ("visits", "value", "prior", "nodes", "sims", "best")
LEAF_KEYS = ("leaf_board", "leaf_heads", "leaf_dirs", "leaf_deaths")


def _batch(st, first_env_id=CASES.FIRST_ENV_ID):
    """a TronBatch holding the oracle state `st`, step counters included"""
    from colosseumrl_amd.batched import TronBatch
    # (the start layout needs a 4x4 board; below that any distinct cells serve: the position is put over them)
    start = None if st.N >= 4 else (list(range(st.P)), [0] * st.P)
    tb = TronBatch(st.N, st.P, st.B, device=DEV, start=start, first_env_id=first_env_id)
    tron_put(tb, st.board, st.heads, st.dirs, st.deaths)
    tb.tcount.copy_(torch.from_numpy(st.tcount.view(np.int32)))
    return tb


def _leaves_np(leaves):
    return {k: (u32_of(v) if k == "depth" else _np(v)) for k, v in leaves.items()}


def _root_np(root):
    return {k: _np(root[k]) if k == "best" else u32_of(root[k]) for k in ROOT_KEYS}


def _same(got, want, what, skip=()):
    for key, w in want.items():
        if key not in skip:
            g = got[key]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, g.shape)
            assert np.array_equal(g, w), (what, key, np.argwhere(g != w)[:6].tolist())


def _eval_to_dev(prior, value):
    return torch.from_numpy(prior.view(np.int16)).to(DEV), torch.from_numpy(value).to(DEV)


def _select_without_leaf(tb, cpuct, fpu, out):
    """crl_tron_puct_select with the leaf_* set NULL (the wrapper always passes one)"""
    from colosseumrl_amd.batched import _ptr
    tb._call("crl_tron_puct_select", _ptr(tb._puct_tree), tb._puct_cap, cpuct, fpu, _ptr(out["obs_board"]), _ptr(out["obs_heads"]),
             _ptr(out["obs_dirs"]), _ptr(out["obs_deaths"]), _ptr(out["pending"]), _ptr(out["depth"]), None, None, None, None, 0)
    return out


def _gpu_run(st, seat, agent, S, S_cap=None, cpuct=256, fpu=32768, mode="mix", extra=0, twice=False, no_leaf=False, between=None,
             noise=CASES.NOISE, first_env_id=CASES.FIRST_ENV_ID, seed=CASES.SEED):
    """the search on a stepper holding `st`, the test evaluator on the host: (stepper, root dict, [select dicts])"""
    tb = _batch(st, first_env_id)
    tb.puct_begin(S_cap or S, seed, agent, noise, None if seat is None else torch.from_numpy(seat).to(DEV))
    seen, leaves = [], None
    for s in range(S + extra):
        if twice:
            first = _leaves_np(tb.puct_select(cpuct / 256, fpu / 65536))
        if no_leaf:
            leaves = leaves or tb.puct_select(cpuct / 256, fpu / 65536)
            for key in LEAF_KEYS:
                leaves[key].fill_(-3)
            got = _leaves_np(_select_without_leaf(tb, cpuct, fpu, leaves))
            assert all((got[key] == -3).all() for key in LEAF_KEYS)              # not written
        else:
            leaves = tb.puct_select(cpuct / 256, fpu / 65536, out=leaves)
            got = _leaves_np(leaves)
        if twice:
            _same(got, first, ("select twice", s))
        seen.append(got)
        tb.puct_backup(*_eval_to_dev(*R.evaluator(got["obs_board"], got["obs_heads"], got["obs_dirs"], mode)))
        if between:
            between(tb, s)
    return tb, _root_np(tb.puct_root()), seen


@functools.lru_cache(maxsize=None)
def _reference(shape, B, S, S_cap=None, cpuct=256, fpu=32768, mode="mix", extra=0):
    """the restatement's root and per-simulation leaves of a case, computed once and shared"""
    N, P, agent = CASES.SHAPES[shape]
    return R.run(CASES.state(N, P, B), S, S_cap, cpuct, fpu, mode, None, True, extra, seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID,
                 seat=CASES.shape_seats(shape, B), agent=agent, noise=CASES.NOISE)


def _compare(shape, B, S, what, **kw):
    N, P, agent = CASES.SHAPES[shape]
    st, seat = CASES.state(N, P, B), CASES.shape_seats(shape, B)
    ref_kw = {key: v for key, v in kw.items() if key in ("S_cap", "cpuct", "fpu", "mode", "extra")}
    want_root, want_seen = _reference(shape, B, S, **ref_kw)
    before = [a.copy() for a in (st.board, st.heads, st.dirs, st.deaths, st.tcount)]
    tb, root, seen = _gpu_run(st, seat, agent, S, **kw)
    assert len(seen) == len(want_seen)
    for s, (g, w) in enumerate(zip(seen, want_seen)):
        _same(g, w, (what, "select", s), skip=LEAF_KEYS if kw.get("no_leaf") else ())
    _same(root, want_root, (what, "root"))
    # the game state is bit-identical after a whole search
    assert all(np.array_equal(a, b) for a, b in zip(tron_state(tb) + [u32_of(tb.tcount)], before))
    return tb, root, seen


# ------------------------------------------------------------------ 1. every shape, B = 1, 5 and 130
@pytest.mark.parametrize("B", CASES.BATCHES)
@pytest.mark.parametrize("shape", range(len(CASES.SHAPES)), ids=CASES.SHAPE_IDS)
def test_matches_the_restatement(shape, B):
    N, P, agent = CASES.SHAPES[shape]
    tb, root, seen = _compare(shape, B, CASES.S_MAIN, (CASES.SHAPE_IDS[shape], B))
    if B == 130:
        assert (root["nodes"] == 0).sum() >= 2 and (root["best"] == -1).sum() >= (root["nodes"] == 0).sum()
        assert (root["sims"][root["nodes"] > 0] == CASES.S_MAIN).all()
        assert any((s["pending"] == 0).sum() > (root["nodes"] == 0).sum() for s in seen)      # terminal leaves among them
        assert max(int(s["depth"].max()) for s in seen) >= (0 if P == 1 else 3)     # (one player: every child is closed, the root alone is pending)


# ------------------------------------------------------------------ 2. the edges, one row each
@pytest.mark.parametrize("case", CASES.EDGE_CASES, ids=[c["id"] for c in CASES.EDGE_CASES])
def test_edges(case):
    kw = {key: case[key] for key in ("S_cap", "cpuct", "fpu", "mode", "extra", "twice", "no_leaf") if key in case}
    tb, root, seen = _compare(case["shape"], 8, case["S"], case["id"], **kw)
    for s in seen[case["S"]:]:                                   # past the capacity: no-ops with pending 0
        assert not s["pending"].any() and not s["obs_board"].any() and not s["depth"].any() and not s["obs_heads"].any()


# ------------------------------------------------------------------ 3. a path deeper than 64 nodes
def test_a_path_deeper_than_64_nodes():
    st, row = CASES.deep_state(), CASES.DEEP
    want_root, want_seen = R.run(st, row["S"], cpuct=row["cpuct"], fpu=row["fpu"], mode=row["mode"], record=True, agent=row["agent"],
                                 noise=row["noise"], seed=3, first_env_id=0)
    tb, root, seen = _gpu_run(st, None, row["agent"], row["S"], cpuct=row["cpuct"], fpu=row["fpu"], mode=row["mode"],
                              noise=row["noise"], first_env_id=0, seed=3)
    for s, (g, w) in enumerate(zip(seen, want_seen)):
        _same(g, w, ("deep", "select", s))
    _same(root, want_root, ("deep", "root"))
    assert [int(s["depth"][0]) for s in seen[:67]] == list(range(67))           # one ply deeper per simulation
    assert root["nodes"][0] == 68 and root["visits"][0].tolist() == [69, 0, 0]  # the path of 68 nodes was backed up three times
    assert root["value"][0, 0] == 65536 * 66                                     # (66 pending leaves below the root's child won)


# ------------------------------------------------------------------ 4. the batch stepped while the search is open
def test_stepping_between_begin_and_root():
    N, P, agent = CASES.SHAPES[1]
    st, seat = CASES.state(N, P, 40), CASES.seats(P, 40)

    def between(tb, s):
        if s % 5 == 0:
            tb.step(tb.sample_avoid(seed=s, advance=True), auto_reset=True)
    tb, root, seen = _gpu_run(st, seat, agent, 40, between=between)
    want_root, want_seen = _reference(1, 40, 40)
    _same(root, want_root, "stepped")
    for s, (g, w) in enumerate(zip(seen, want_seen)):            # every select: a read of the live state would show at once
        _same(g, w, ("stepped", "select", s))
    assert not np.array_equal(_np(tb.board), st.board)           # the games did move


# ------------------------------------------------------------------ 5. select -> evaluator on the device -> backup in one graph
def test_graph_replay_equals_the_eager_run():
    N, P, agent = CASES.SHAPES[1]
    st, seat, S = CASES.state(N, P, 70), torch.from_numpy(CASES.seats(P, 70)).to(DEV), 40
    eager = _batch(st)
    want = _root_np(eager.puct(_device_evaluator, S, seed=5, agent=agent, noise=CASES.NOISE, seat=seat))
    assert (want["sims"][want["nodes"] > 0] == S).all()
    tb = _batch(st)
    tb.puct_begin(S, 5, agent, CASES.NOISE, seat)
    leaves = tb.puct_select()

    def pair():
        tb.puct_select(out=leaves)
        tb.puct_backup(*_device_evaluator(leaves))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on a side stream, as torch.cuda.graph wants
        pair()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                    # one stream, one chain: no parallel branches
        pair()
    tb.puct_begin(S, 5, agent, CASES.NOISE, seat)                # the warm-up was a simulation: start again
    for _ in range(S):
        g.replay()
    torch.cuda.synchronize()
    _same(_root_np(tb.puct_root()), want, "graph")


# ------------------------------------------------------------------ 6. the wrappers: `out` reuse, puct / puct_action, the vector env
def test_wrappers():
    N, P, agent = CASES.SHAPES[0]
    st = CASES.state(N, P, 8)
    tb = _batch(st)
    want, _ = R.run(st, 20, cpuct=R.cpuct_of(1.25), mode="uniform", seed=9, first_env_id=CASES.FIRST_ENV_ID, agent="avoid", noise=0.5)
    prior, value = torch.ones((8, 3)), torch.full((8,), 0.5)      # float: quantised by puct
    out = tb.puct(lambda leaves: (prior.to(DEV), value.to(DEV)), 20, seed=9, agent="avoid", noise=0.5)
    _same(_root_np(out), want, "puct")
    tree = tb._puct_tree
    again = tb.puct(lambda leaves: (prior.to(DEV), value.to(DEV)), 20, seed=9, agent="avoid", noise=0.5, out=out)
    assert all(again[key] is out[key] for key in out) and tb._puct_tree is tree       # the trees and the dict are reused
    _same(_root_np(again), want, "puct again")
    act = tb.puct_action(lambda leaves: (prior.to(DEV), value.to(DEV)), 20, seed=9, agent="avoid", noise=0.5)
    assert act.dtype == torch.int64 and np.array_equal(_np(act), want["best"].astype(np.int64))
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    env = TronSinglePlayerVectorEnv(9, 3, 16, noise=0.25, seed=4, device=DEV)
    env.reset()
    p16, v16 = torch.ones((16, 3), device=DEV), torch.full((16,), 0.5, device=DEV)
    a = env.puct_action(lambda leaves: (p16, v16), 12)
    b = env.batch.puct_action(lambda leaves: (p16, v16), 12, 1.25, 0.5, 1, "avoid", 0.25, None)
    assert a.dtype == torch.int64 and torch.equal(a, b) and bool(((a >= 0) & (a <= 2)).all())


# ------------------------------------------------------------------ 7. rows below one 16-byte chunk, rows at odd byte offsets
def _compare_state(st, seat, agent, S, what, **kw):
    """a search on the state `st` (not one of the table's shapes) against the restatement: every select and the root"""
    ref_kw = {key: kw[key] for key in ("S_cap", "cpuct", "fpu", "mode", "extra") if key in kw}
    want_root, want_seen = R.run(st, S, count=None, record=True, seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID, seat=seat, agent=agent,
                                 noise=kw.get("noise", CASES.NOISE), **ref_kw)
    before = [a.copy() for a in (st.board, st.heads, st.dirs, st.deaths, st.tcount)]
    tb, root, seen = _gpu_run(st, seat, agent, S, **kw)
    assert len(seen) == len(want_seen)
    for s, (g, w) in enumerate(zip(seen, want_seen)):
        _same(g, w, (what, "select", s))
    _same(root, want_root, (what, "root"))
    assert all(np.array_equal(a, b) for a, b in zip(tron_state(tb) + [u32_of(tb.tcount)], before))
    return root, seen


@pytest.mark.parametrize("row", CASES.tiny_states(), ids=[row[0] for row in CASES.tiny_states()])
def test_boards_below_16_cells(row):
    name, st, seat, agent, noise = row
    root, seen = _compare_state(st, seat, agent, CASES.TINY_S, name, noise=noise)
    assert (root["nodes"] > 0).all() and seen[0]["pending"].all()


@pytest.mark.parametrize("off", [1, 7, 15])
@pytest.mark.parametrize("shape", [15, 7], ids=[CASES.SHAPE_IDS[i] for i in (15, 7)])
def test_output_rows_at_odd_byte_offsets(shape, off):
    """`obs_board` and `leaf_board` as views that start `off` and 16 - `off` bytes behind a 16-byte boundary of a larger buffer
    (4x4: a row is one chunk and never aligned; 7x7: 49 bytes): the rows as the restatement has them, the guard bytes before and
    behind the views untouched"""
    N, P, agent = CASES.SHAPES[shape]
    B, S, NN, G = 8, 20, N * N, 64
    want_root, want_seen = _reference(shape, B, S)
    tb = _batch(CASES.state(N, P, B))
    tb.puct_begin(S, CASES.SEED, agent, CASES.NOISE, torch.from_numpy(CASES.shape_seats(shape, B)).to(DEV))
    bufs = {key: torch.full((G + B * NN + G,), -7, dtype=torch.int8, device=DEV) for key in ("obs_board", "leaf_board")}
    at = {"obs_board": 32 + off, "leaf_board": 48 - off}
    out = {key: torch.empty(dims, dtype=dt, device=DEV) for key, (dt, dims) in tb._puct_select_spec().items()}
    for key, buf in bufs.items():
        assert buf.data_ptr() % 16 == 0
        out[key] = buf[at[key]:at[key] + B * NN].view(B, NN)
        assert out[key].data_ptr() % 16 == at[key] % 16 and out[key].is_contiguous()
    for s in range(S):
        got = _leaves_np(tb.puct_select(1.0, 0.5, out=out))       # (cpuct 256, fpu 32768: the reference's)
        _same(got, want_seen[s], ("offset", off, "select", s))
        for key, buf in bufs.items():
            assert bool((buf[:at[key]] == -7).all()) and bool((buf[at[key] + B * NN:] == -7).all()), (key, s)
        tb.puct_backup(*_eval_to_dev(*R.evaluator(got["obs_board"], got["obs_heads"], got["obs_dirs"])))
    _same(_root_np(tb.puct_root()), want_root, ("offset", off, "root"))


# ------------------------------------------------------------------ 8. the workgroup shapes of `select`: 4, 3, 2 waves and 1, up to 64 KB of LDS
@pytest.mark.parametrize("N, P, B", CASES.LDS_CASES, ids=CASES.LDS_IDS)
def test_every_workgroup_shape_of_select(N, P, B):
    """127 | 128, 147 | 148, 180 | 181: the boards on either side of each change of the wave count (tests/test_tron_puct_host.py
    restates the rule), B = 5 so that the last workgroup is ragged with 4, 3 and 2 waves; 181x181 has heads in the last row
    and the last column"""
    st, seat = CASES.lds_state(N, P, B)
    root, seen = _compare_state(st, seat, "avoid", CASES.LDS_S, (N, P, B))
    assert (root["sims"] == CASES.LDS_S).all()


# ------------------------------------------------------------------ 9. trees of the greatest capacity
@pytest.mark.parametrize("row", CASES.CAPACITY, ids=[row["id"] for row in CASES.CAPACITY])
def test_trees_at_capacity(row):
    """20x20 from the start layout, S = S_cap: 4,095 at the default exploration (trees of 3,860 and 3,789 nodes, 19 plies,
    n up to 3,584), 1,024 at cpuct = 65,535; every select and the root, then two pairs past the capacity"""
    st, S = CASES.capacity_state(), row["S"]
    root, seen = _compare_state(st, None, "avoid", S, row["id"], cpuct=row["cpuct"], noise=CASES.CAPACITY_NOISE, extra=CASES.CAPACITY_EXTRA)
    assert int(root["nodes"].max()) >= row["reaches"]["nodes"] and (root["sims"] == S).all()
    for s in seen[S:]:
        assert not s["pending"].any() and not s["obs_board"].any() and not s["depth"].any() and not s["obs_heads"].any()


# ------------------------------------------------------------------ 10. the step's killer ids
@pytest.mark.parametrize("agent", ["random", "avoid"])
@pytest.mark.parametrize("N, P", CASES.CRASH_CASES, ids=["%dx%dp%d" % (N, N, P) for N, P in CASES.CRASH_CASES])
def test_the_crash_rows(N, P, agent):
    """the rows on which tests/test_tron_puct_host.py counts every crash kind above a pending leaf: the killer ids go out in
    leaf_deaths and obs_deaths"""
    st, seat = CASES.state(N, P, CASES.CRASH_B), CASES.crash_seats(P, CASES.CRASH_B)
    root, seen = _compare_state(st, seat, agent, CASES.CRASH_S, ("crash", N, P, agent))
    assert any(s["leaf_deaths"][:, s["pending"] == 1].any() for s in seen)


# ------------------------------------------------------------------ 11. strength, through the product
def _first_episode_wins(policy, games, seed=5, max_t=300):
    """the share of first episodes the learner wins in TronSinglePlayerVectorEnv(15, 4, noise 0.1)"""
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    env = TronSinglePlayerVectorEnv(15, 4, games, noise=0.1, seed=seed, device=DEV)
    env.reset()
    reward, _, _ = first_episodes(env, policy, max_t)
    return float((reward == 10).double().mean())                # +10: the surviving winner, on the step that ends the game


def _avoid_policy(env, t):
    act = env.batch.sample_avoid(99, env.noise, players=[0], advance=False)[0].to(torch.int64)
    return torch.where(act < 0, 2, act)


def test_territory_valued_puct_learner_beats_the_avoid_learner():
    """15x15, the learner against three avoid agents (noise 0.1), G = 256 games on the same seeds, first episodes.  The learner
    plays puct_action(48) with uniform priors; the value of a leaf is the territory share a_s / (a_s + a_o) of
    TronBatch.territory on the leaf_* state in a second stepper (a_s the seat's area, a_o the best other live player's; 0.5
    when nobody has any).  Its win rate must exceed the avoid learner's by more than three standard errors of the difference
    of two binomials at the measured rates."""
    from colosseumrl_amd.batched import TronBatch
    G = 256
    scratch = TronBatch(15, 4, G, device=DEV)
    ones = torch.ones((G, 3), device=DEV)

    def evaluate(leaves):
        scratch.board.copy_(leaves["leaf_board"]), scratch.heads.copy_(leaves["leaf_heads"])
        scratch.dirs.copy_(leaves["leaf_dirs"]), scratch.deaths.copy_(leaves["leaf_deaths"])
        area = scratch.territory()["area"][:, 0, :].float()                      # [G, P]; dead players hold 0
        a_s, a_o = area[:, 0], area[:, 1:].amax(dim=1)
        den = a_s + a_o
        return ones, torch.where(den > 0, a_s / den.clamp_min(1.0), torch.full_like(den, 0.5))

    puct = _first_episode_wins(lambda env, t: env.puct_action(evaluate, 48, seed=1000 + t), G)
    avoid = _first_episode_wins(_avoid_policy, G)
    se = math.sqrt(puct * (1.0 - puct) / G + avoid * (1.0 - avoid) / G)
    print("\nfirst-episode win rate over %d games: puct_action(48) valued by territory %.4f, avoid learner %.4f, "
          "difference %.4f = %.1f standard errors" % (G, puct, avoid, puct - avoid, (puct - avoid) / max(se, 1e-12)))
    assert puct - avoid > 3.0 * se, (puct, avoid, se)
