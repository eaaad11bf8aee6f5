"""Batched tree search for a seat of Tron (crl_tron_mcts) on the host: the argument checks of the two C entries (every
CRL_EINVAL / CRL_EUNSUPPORTED case is refused with its message before any device work), S_max per board, the argument checks
of the Python wrappers, and the plain-Python restatement of the header's contract (tests/tron_mcts_ref.py) -- its own step,
agents and playout held to the oracle and to tests/tron_ref.py, and hand-made answers."""
import numpy as np
import pytest

from tests import rng_ref as RNG
from tests import tron_mcts_ref as M
from tests import tron_mcts_territory_ref as T
from tests import tron_ref as TR
from tests.host_util import D, fake as _fake, lib as _lib, tron_context, ttt_context


def _call(lib, ctx, B=4, state=(D,) * 4, tcount=D, seat=D, S=8, Rn=4, cexp=256, noise=0.1, max_steps=0, outs=(D,) * 4, flags=0):
    return lib.crl_tron_mcts(ctx, B, 1, 0, *state, tcount, seat, S, Rn, cexp, noise, max_steps, *outs, flags, None)


def test_mcts_argument_checks():
    lib = _lib()
    with tron_context() as h, ttt_context() as tt:
        for i in range(4):                 # board, heads, dirs, deaths (tcount and seat may be NULL)
            st = [D] * 4
            st[i] = None
            assert _call(lib, h, state=tuple(st)) == -1 and b"NULL state" in lib.crl_last_error()
        for i in range(4):
            outs = [D] * 4
            outs[i] = None
            assert _call(lib, h, outs=tuple(outs)) == -1 and b"NULL output" in lib.crl_last_error()
        for B in (0, -1, (1 << 31) + 1):
            assert _call(lib, h, B=B) == -1 and b"B=" in lib.crl_last_error()
        for S in (0, -1, 4079, 4096, 1 << 30):
            assert _call(lib, h, S=S) == -1 and b"S=" in lib.crl_last_error()
        for Rn in (0, -3, 1025, 65535):
            assert _call(lib, h, Rn=Rn) == -1 and b"R=" in lib.crl_last_error()
        for cexp in (65536, 0xFFFFFFFF):
            assert _call(lib, h, cexp=cexp) == -1 and b"cexp=" in lib.crl_last_error()
        for noise in (-0.01, 1.0001, float("nan"), float("inf")):
            assert _call(lib, h, noise=noise) == -1 and b"noise" in lib.crl_last_error()
        for ms in (-1, 65536):
            assert _call(lib, h, max_steps=ms) == -1 and b"max_steps" in lib.crl_last_error()
        for flags in (2, 3, 8, 0x80000000):           # CRL_PLAYOUT_AVOID (1) only
            assert _call(lib, h, flags=flags) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, None) == -1 and b"tron context" in lib.crl_last_error()
        assert _call(lib, tt) == -1 and b"tron context" in lib.crl_last_error()
        assert lib.crl_tron_mcts_max_simulations(None) == -1 and b"tron context" in lib.crl_last_error()
        assert lib.crl_tron_mcts_max_simulations(tt) == -1 and b"tron context" in lib.crl_last_error()


@pytest.mark.parametrize("N", [90, 128, 181])
def test_unsupported_boards(N):
    """S_max below 1: both entries answer CRL_EUNSUPPORTED (-4), whatever S"""
    lib = _lib()
    assert M.max_simulations(N) < 1
    with tron_context(N, 2, (0, N * N - 1), (2, 0)) as h:
        assert lib.crl_tron_mcts_max_simulations(h) == -4 and b"LDS" in lib.crl_last_error()
        assert _call(lib, h, S=1) == -4 and b"LDS" in lib.crl_last_error()
        assert _call(lib, h, state=(None, D, D, D)) == -1    # (the NULL checks come first, as everywhere)


@pytest.mark.parametrize("N, s_max", [(4, 4078), (5, 4078), (19, 3897), (20, 3880), (40, 3270), (64, 1983), (89, 3)])
def test_max_simulations(N, s_max):
    """S_max = min(4095, (65536 - 264 nwords) / 16 - 1): S_max + 1 nodes and 66 bitboards fit 64 KB, one node more does not;
    S_max passes the check of S, S_max + 1 does not.  (The call with S_max is stopped by a later check -- the flags -- so
    that nothing is launched on the dummy pointers.)"""
    lib = _lib()
    assert M.max_simulations(N) == s_max
    assert M.wave_bytes(N, s_max) <= 65536 < M.wave_bytes(N, s_max + 1) or s_max == 4095
    with tron_context(N, 2, (0, N * N - 1), (2, 0)) as h:
        assert lib.crl_tron_mcts_max_simulations(h) == s_max
        assert _call(lib, h, S=s_max, flags=2) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, h, S=s_max + 1, flags=2) == -1 and b"S=" in lib.crl_last_error()


def test_max_simulations_conditions():
    """the issue's two conditions: at least 2048 up to 20x20, at least 512 up to 64x64; and s < 4095 everywhere"""
    assert all(M.max_simulations(N) >= 2048 for N in range(2, 21))
    assert all(M.max_simulations(N) >= 512 for N in range(2, 65))
    assert all(M.max_simulations(N) <= 4095 for N in range(2, 182))
    assert [N for N in range(2, 182) if M.max_simulations(N) < 1] == list(range(90, 182))


def test_mcts_prototypes_and_tags():
    """revision 113, the two entries bound, and no Philox tag beyond the twelve of tests/rng_ref.py"""
    import os
    import re
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    assert "crl_tron_mcts" in _native.PROTOTYPES and "crl_tron_mcts_max_simulations" in _native.PROTOTYPES
    assert len(_native.PROTOTYPES["crl_tron_mcts"][1]) == 21
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = open(os.path.join(root, "colosseumrl_amd", "csrc", "crl_common.hpp")).read()
    assert len(re.findall(r"#define\s+CRL_TAG_\w+\s+0x[0-9a-fA-F]+u", common)) == len(RNG.TAGS) == 12
    assert M.TREE_STEP >> 16 == 0xFFFF                       # beyond crl_tron_playout's a < 65535 and the leaves' s <= 4094


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TronBatch
    tb = _fake(TronBatch, B=5, P=3, N=7)
    tb.__dict__["mcts_max_simulations"] = 4046
    for fn in (tb.mcts, tb.mcts_action):
        for bad in (0, 4047, -1, 2.0, True, None):
            with pytest.raises(ValueError):
                fn(bad)
        for bad in (0, 1025, 16.0, False):
            with pytest.raises(ValueError):
                fn(8, bad)
        for bad in (-0.5, 256.0, float("nan"), "1", True, None):
            with pytest.raises(ValueError):
                fn(8, 16, 0, bad)
        for kw in ({"agent": "greedy"}, {"agent": None}, {"noise": -0.5}, {"noise": 1.5}, {"noise": float("nan")},
                   {"noise": "0.1"}, {"max_steps": -1}, {"max_steps": 65536}, {"max_steps": 2.0},
                   {"seat": torch.zeros((5,), dtype=torch.int32)}, {"seat": torch.zeros((4,), dtype=torch.int8)},
                   {"seat": np.zeros(5, np.int8)}):
            with pytest.raises(ValueError):
                fn(8, **kw)
    i32 = torch.int32
    good = {"visits": torch.zeros((5, 3), dtype=i32), "value": torch.zeros((5, 3), dtype=i32),
            "nodes": torch.zeros((5,), dtype=i32), "best": torch.zeros((5,), dtype=i32)}
    for key, wrong in (("visits", torch.zeros((5, 4), dtype=i32)), ("value", torch.zeros((5, 3), dtype=torch.int64)),
                       ("nodes", torch.zeros((4,), dtype=i32)), ("best", torch.zeros((5,), dtype=torch.int64))):
        with pytest.raises(ValueError):
            tb.mcts(8, out=dict(good, **{key: wrong}))
        with pytest.raises(ValueError):
            tb.mcts(8, out={k: v for k, v in good.items() if k != key})


def test_vector_env_wrapper_argument_checks():
    from colosseumrl_amd.batched import TronBatch
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    env = TronSinglePlayerVectorEnv.__new__(TronSinglePlayerVectorEnv)
    env.batch, env.noise = _fake(TronBatch, B=5, P=4, N=15), 0.1
    env.batch.__dict__["mcts_max_simulations"] = 3000
    for args in ((0,), (3001,), (8, 0), (8, 1025), (8, 16, 1, -1.0), (8, 16, 1, 1.0, -1), (8, 16, 1, 1.0, 65536)):
        with pytest.raises(ValueError):
            env.mcts_action(*args)


# ---- the restatement: its parts against the oracle and tests/tron_ref.py
def _one(st, b):
    """game b of an oracle state as a state of its own"""
    from oracle import oracle as O
    one = O.TronState(st.N, st.P, 1)
    one.board[0], one.heads[:, 0], one.dirs[:, 0], one.deaths[:, 0] = st.board[b], st.heads[:, b], st.dirs[:, b], st.deaths[:, b]
    return one


def _same(pos, one):
    return (pos.board == one.board[0].tolist() and pos.h == one.heads[:, 0].tolist() and pos.d == one.dirs[:, 0].tolist()
            and pos.k == one.deaths[:, 0].tolist())


@pytest.mark.parametrize("N, P", [(5, 2), (7, 3), (9, 8), (13, 4)])
@pytest.mark.parametrize("agent", ["random", "avoid"])
def test_tree_step_matches_oracle_and_tron_ref(N, P, agent):
    """the restatement's tree step == oracle.tron_step on tron_ref's agents under the third word 0xFFFF0000, the seat's row
    overwritten; chains of tree steps, so that dead players and head-on hits occur"""
    from oracle import oracle as O
    rng = np.random.default_rng(N * 10 + P)
    B, seed, noise, first = 12, 0xC0FFEE12345, 0.3, (1 << 32) + 5
    st = M.positions(N, P, B, rng)
    k0, k1, thr = seed & RNG.M32, (seed >> 32) & RNG.M32, RNG.threshold(noise)
    stepped = 0
    for b in range(B):
        seat = int(rng.integers(0, P))
        one, pos = _one(st, b), M.pos_of(st, b)
        g, c = (first + b) & RNG.M32, int(st.tcount[b])
        for k in range(6):
            if one.deaths[seat, 0] != 0:
                break
            e = int(rng.integers(0, 3))
            ga, ca = np.array([g], np.uint32), np.array([c], np.uint32)
            if agent == "avoid":
                act = TR.decide(N, one.board, one.heads, one.dirs, one.deaths, ga, ca, seed, noise,
                                c2=np.array([M.TREE_STEP], np.uint32), tag=RNG.CRL_TAG_TRON_AVOID_PLAYOUT, occupied=TR.positive)
            else:
                act = TR.random_actions(P, ga, ca, np.array([M.TREE_STEP], np.uint32), seed)
            act[seat, 0] = (0, 1, -1)[e]
            _, term, win = O.tron_step(one, act)
            t2, w2 = M.tree_step(N, pos, seat, e, agent, thr, k0, k1, g, c)
            assert _same(pos, one) and (bool(term[0]), int(win[0])) == (t2, w2)
            assert M.is_closed(pos, seat) == (one.deaths[seat, 0] != 0 or (one.deaths[:, 0] == 0).sum() <= 1)
            c = (c + 1) & RNG.M32
            stepped += 1
    assert stepped > B                                        # (not vacuous: more than one step per game on average)


@pytest.mark.parametrize("N, P", [(5, 2), (7, 3), (9, 5)])
@pytest.mark.parametrize("agent, max_steps", [("random", 0), ("avoid", 0), ("avoid", 4)])
def test_playout_matches_tron_ref(N, P, agent, max_steps):
    """the restatement's playout at s = 0 == tron_ref.tron_playout(cand=None) stopped with the seat: the seat's wins are the
    playouts worth 2 half-points, the steps are len_sum; a capped playout with the seat alive is worth 1"""
    rng = np.random.default_rng(N + P)
    B, Rn, seed, noise, first = 8, 6, 77, 0.2, (1 << 32) - 3
    st = M.positions(N, P, B, rng)
    seat = rng.integers(0, P, size=B)
    wins, played, len_sum, _ = TR.tron_playout(st, seed, Rn, seat=seat, tcount=st.tcount, first_env_id=first, agent=agent,
                                               noise=noise, until="seat_done", max_steps=max_steps)
    k0, k1, thr = seed & RNG.M32, (seed >> 32) & RNG.M32, RNG.threshold(noise)
    n_played = 0
    for b in range(B):
        if not played[b, 0]:
            continue
        count = M.new_count()
        hp = [M.playout(N, M.pos_of(st, b), int(seat[b]), agent, thr, k0, k1, (first + b) & RNG.M32, int(st.tcount[b]), r,
                        max_steps, count) for r in range(Rn)]
        assert hp.count(2) == wins[b, 0, seat[b]] and count["steps"] == len_sum[b, 0] and count["playouts"] == Rn
        assert max_steps or 1 not in hp
        n_played += 1
    assert n_played >= B // 2


# ---- hand-made answers
def _state(N, P, heads, dirs, walls=(), B=1):
    from oracle import oracle as O
    st = O.TronState(N, P, B)
    for b in range(B):
        st.board[b, list(walls)] = 1
        for p in range(P):
            st.board[b, heads[p]] = p + 1
            st.heads[p, b], st.dirs[p, b] = heads[p], dirs[p]
    return st


@pytest.mark.parametrize("agent", ["random", "avoid"])
def test_single_player_every_child_closed(agent):
    """P = 1 on 5x5: every tree step is terminal, so every child is closed and no draw is made.  From the corner (0, 0)
    facing east: forward and right survive, left leaves the board.  S = 3 visits each once with 2R or 0; with cexp = 0 every
    later visit goes to the lowest surviving action."""
    Rn = 5
    st = _state(5, 1, [0], [1], B=2)
    st.dirs[0, 1] = 0                                         # game 1 faces north: forward and left leave the board
    count = M.new_count()
    v, w, n, best = M.tron_mcts(st, 3, Rn, cexp=0, agent=agent, count=count)
    assert v.tolist() == [[1, 1, 1], [1, 1, 1]] and w.tolist() == [[2 * Rn, 2 * Rn, 0], [0, 2 * Rn, 0]]
    assert n.tolist() == [4, 4] and best.tolist() == [0, 1] and count["playouts"] == 0 and count["closed"] == 6
    v, w, n, best = M.tron_mcts(st, 20, Rn, cexp=0, agent=agent, seed=9, tcount=np.array([7, 2 ** 32 - 1], np.uint32))
    assert v.tolist() == [[18, 1, 1], [1, 18, 1]] and w.tolist() == [[36 * Rn, 2 * Rn, 0], [0, 36 * Rn, 0]]
    assert n.tolist() == [4, 4] and best.tolist() == [0, 1]
    # with exploration the other surviving action is visited too, the fatal one as well, and nothing else is ever made
    v, w, n, best = M.tron_mcts(st, 200, Rn, cexp=256, agent=agent)
    assert n.tolist() == [4, 4] and v.sum(axis=1).tolist() == [200, 200] and (v > 1).sum(axis=1).tolist() == [3, 3]
    assert (w[:, 2] == 0).all() and w[0, 0] == 2 * Rn * v[0, 0] and w[0, 1] == 2 * Rn * v[0, 1]


def test_search_avoids_the_pocket():
    """9x9, two players.  The seat stands at (4, 4) facing north; ahead lies a pocket of three cells between two walls, to
    its left a wall, to its right the open board; the opponent is far away.  Forward lives three more steps, so against the
    avoid agent its playouts are lost; the search prefers the open side from a dozen simulations on."""
    N = 9
    walls = [y * N + x for y in (1, 2, 3) for x in (3, 5)] + [0 * N + 4, 4 * N + 3, 5 * N + 4]
    st = _state(N, 2, [4 * N + 4, 8 * N + 8], [0, 3], walls)
    for S in (12, 48):
        v, w, n, best = M.tron_mcts(st, S, 8, agent="avoid", noise=0.0, seed=S)
        assert best[0] == 1 and v[0, 1] > v[0, 0] >= 1 and v[0, 2] >= 1
        assert w[0, 0] == 0 and w[0, 2] == 0 and w[0, 1] > 0 and n[0] > 4 and v[0].sum() == S


@pytest.mark.parametrize("S", [3, 64])
def test_step_rule_corners_by_hand(S):
    """The step rule's sharp corners on positions whose values can be worked out on paper (avoid model, noise 0, R = 4;
    tests/tron_mcts_territory_ref.py draws the boards).

    Head-on: player 0 at (1, 3) heading east, player 1 at (3, 3) heading west, the one free cell (2, 3) between them.  The
    model player steps forward (its cell ahead is free).  If the seat steps forward too, the lower player takes (2, 3) and the
    higher one runs into that head: the mover dies and, the cell being the other's head, so does its owner -- whichever of
    the two the seat is, it is dead: the forward child is closed and worth 0 at every visit.  If the seat turns into its own
    column, the model player stands in (2, 3) with the seat's trail ahead and walls on both sides and dies on the next step,
    the seat (forward along its column) survives it alone: each of the R playouts is worth 2.  So S = 3 gives [0, 2R, 2R].

    The bystander: players 0 and 1 kill each other in every first tree step, seat 2 moves onto a free cell whichever way it
    turns and is alone alive: three closed, won children and never a fourth node.

    The corner: the seat at (0, 0) heading north; forward and left leave the board (closed, 0).  To the right it has five
    more cells of the top row, the other player two more of its three: on the third playout step the other player dies, the
    seat wins: 2R."""
    Rn = 4
    seats = lambda s: np.array([s], np.int8)
    for seat in (0, 1):                                       # the seat moves first, the seat moves second
        count = M.new_count()
        v, w, n, best = M.tron_mcts(T.head_on_state(), S, Rn, seat=seats(seat), agent="avoid", noise=0.0, count=count)
        assert w[0, 0] == 0 and best[0] != 0 and v[0].sum() == S and v[0, 0] >= 1
        assert count["head_on"] == 1 and count["closed"] >= v[0, 0]     # (one hit on a head: the expansion of the forward child)
        if S == 3:
            assert w.tolist() == [[0, 2 * Rn, 2 * Rn]] and n.tolist() == [4] and best.tolist() == [1]
    count = M.new_count()
    v, w, n, best = M.tron_mcts(T.head_on_state(3), S, Rn, seat=seats(2), agent="avoid", noise=0.0, count=count)
    assert n.tolist() == [4] and (w == 2 * Rn * v).all() and v[0].sum() == S and (v >= 1).all()
    assert count["head_on"] == 3 and count["playouts"] == 0 and count["closed"] == S
    v, w, n, best = M.tron_mcts(T.corner_state(), S, Rn, agent="avoid", noise=0.0)
    assert w[0, 0] == 0 and w[0, 2] == 0 and best.tolist() == [1] and v[0].sum() == S
    if S == 3:
        assert w.tolist() == [[0, 2 * Rn, 0]]


def test_skipped_positions():
    st = _state(7, 3, [8, 40, 26], [1, 3, 0], B=5)
    st.deaths[1, 1] = 3                                       # b = 1: the seat (player 1) is dead
    st.deaths[0, 2] = 1; st.deaths[2, 2] = 2                  # b = 2: one player alive
    seat = np.array([0, 1, 1, 3, -1])                         # b = 3, 4: seat out of range
    v, w, n, best = M.tron_mcts(st, 6, 3, seat=seat)
    assert n.tolist() == [7, 0, 0, 0, 0] and best[1:].tolist() == [-1] * 4 and best[0] in (0, 1, 2)
    assert (v[1:] == 0).all() and (w[1:] == 0).all() and v[0].sum() == 6


def test_tree_properties():
    """what any such tree has: one node per simulation at most, the root's children sum to S, half-points within 2R per
    visit; the search reads the state and writes none of it"""
    rng = np.random.default_rng(3)
    st = M.positions(7, 3, 6, rng)
    before = [x.copy() for x in (st.board, st.heads, st.dirs, st.deaths, st.tcount)]
    count = M.new_count()
    S, Rn = 24, 3
    v, w, n, best = M.tron_mcts(st, S, Rn, tcount=st.tcount, agent="avoid", max_steps=5, count=count)
    assert all(np.array_equal(a, b) for a, b in zip(before, (st.board, st.heads, st.dirs, st.deaths, st.tcount)))
    played = n > 0
    assert played.any() and (n[played] <= S + 1).all() and (v[played].sum(axis=1) == S).all()
    assert (w <= 2 * Rn * v).all() and ((best >= 0) == played).all()
    assert count["playouts"] == Rn * (S * int(played.sum()) - count["closed"]) and count["steps"] <= 5 * count["playouts"]
