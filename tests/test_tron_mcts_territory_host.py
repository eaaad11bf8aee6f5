"""Tron tree search with Voronoi territory at the leaves (crl_tron_mcts_territory) on the host: the argument checks of the C
entry (every CRL_EINVAL / CRL_EUNSUPPORTED case is refused with its message before any device work), the board widths, the
prototype, the argument checks of the Python wrappers, and the plain-Python restatement of the header's contract
(tests/tron_mcts_territory_ref.py) -- its three area restatements held to each other, and hand-made answers."""
import numpy as np
import pytest

from tests import territory_ref as TV
from tests import tron_mcts_ref as M
from tests import tron_mcts_territory_ref as T
from tests.host_util import D, fake as _fake, lib as _lib, tron_context, ttt_context


def _call(lib, ctx, B=4, state=(D,) * 4, tcount=D, seat=D, S=8, V=256, cexp=256, noise=0.1, outs=(D,) * 4, flags=0):
    return lib.crl_tron_mcts_territory(ctx, B, 1, 0, *state, tcount, seat, S, V, cexp, noise, *outs, flags, None)


def test_argument_checks():
    lib = _lib()
    with tron_context() as h, ttt_context() as tt:
        s_max = lib.crl_tron_mcts_max_simulations(h)
        assert s_max == M.max_simulations(5)
        for i in range(4):                 # board, heads, dirs, deaths (tcount and seat may be NULL)
            st = [D] * 4
            st[i] = None
            assert _call(lib, h, state=tuple(st)) == -1 and b"crl_tron_mcts_territory: NULL state" in lib.crl_last_error()
        for i in range(4):
            outs = [D] * 4
            outs[i] = None
            assert _call(lib, h, outs=tuple(outs)) == -1 and b"crl_tron_mcts_territory: NULL output" in lib.crl_last_error()
        for B in (0, -1, (1 << 31) + 1):
            assert _call(lib, h, B=B) == -1 and b"B=" in lib.crl_last_error()
        for S in (0, s_max + 1, -1, 4096):
            assert _call(lib, h, S=S) == -1 and b"S=" in lib.crl_last_error()
        for V in (0, 1025, -1):
            assert _call(lib, h, V=V) == -1 and b"V=" in lib.crl_last_error()
        for cexp in (65536, 0xFFFFFFFF):
            assert _call(lib, h, cexp=cexp) == -1 and b"cexp=" in lib.crl_last_error()
        for noise in (-0.01, 1.0001, float("nan"), float("inf")):
            assert _call(lib, h, noise=noise) == -1 and b"noise" in lib.crl_last_error()
        for flags in (2, 3, 4, 0x80000000):           # CRL_PLAYOUT_AVOID (1) only
            assert _call(lib, h, flags=flags) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, None) == -1 and b"tron context" in lib.crl_last_error()
        assert _call(lib, tt) == -1 and b"tron context" in lib.crl_last_error()
        # the largest arguments pass every check before the flags (nothing is launched on the dummy pointers)
        assert _call(lib, h, S=s_max, V=1024, cexp=65535, noise=1.0, flags=2) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, h, S=1, V=1, cexp=0, noise=0.0, tcount=None, seat=None, flags=2) == -1 and b"flags" in lib.crl_last_error()


@pytest.mark.parametrize("N", [65, 89, 90, 181])
def test_boards_wider_than_64_are_unsupported(N):
    lib = _lib()
    with tron_context(N, 2, (0, N * N - 1), (2, 0)) as h:
        assert _call(lib, h, S=1) == -4 and b"wider than 64" in lib.crl_last_error()
        assert _call(lib, h, state=(None, D, D, D)) == -1      # (the NULL checks come first, as everywhere)


@pytest.mark.parametrize("N", [2, 32, 33, 64])
def test_boards_up_to_64_pass_the_board_check(N):
    """... with crl_tron_mcts's S_max: S_max passes the check of S, S_max + 1 does not (the flags stop the call)"""
    lib = _lib()
    with tron_context(N, 2, (0, N * N - 1), (2, 0)) as h:
        s_max = lib.crl_tron_mcts_max_simulations(h)
        assert s_max == M.max_simulations(N) and T.wave_bytes(N, s_max) <= 65536
        assert _call(lib, h, S=s_max, flags=2) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, h, S=s_max + 1, flags=2) == -1 and b"S=" in lib.crl_last_error()


def test_prototype():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    assert len(_native.PROTOTYPES["crl_tron_mcts_territory"][1]) == 20
    assert len(_native.PROTOTYPES["crl_tron_mcts"][1]) == 21


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TronBatch
    tb = _fake(TronBatch, B=5, P=3, N=7)
    tb.__dict__["mcts_max_simulations"] = 4046
    for fn in (tb.mcts_territory, tb.mcts_territory_action):
        for bad in (0, 4047, -1, 2.0, True, None):
            with pytest.raises(ValueError):
                fn(bad)
        for bad in (-0.5, 256.0, float("nan"), "1", True, None):
            with pytest.raises(ValueError):
                fn(8, 0, bad)
        for kw in ({"agent": "greedy"}, {"agent": None}, {"noise": -0.5}, {"noise": 1.5}, {"noise": float("nan")},
                   {"noise": "0.1"}, {"value_scale": 0}, {"value_scale": 1025}, {"value_scale": 256.0}, {"value_scale": True},
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
            tb.mcts_territory(8, out=dict(good, **{key: wrong}))
        with pytest.raises(ValueError):
            tb.mcts_territory(8, out={k: v for k, v in good.items() if k != key})


def test_vector_env_wrapper_argument_checks():
    from colosseumrl_amd.batched import TronBatch
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    env = TronSinglePlayerVectorEnv.__new__(TronSinglePlayerVectorEnv)
    env.batch, env.noise = _fake(TronBatch, B=5, P=4, N=15), 0.1
    env.batch.__dict__["mcts_max_simulations"] = 3000
    for args in ((0,), (3001,), (8.0,), (8, 1, -1.0), (8, 1, 256.0)):
        with pytest.raises(ValueError):
            env.mcts_territory_action(*args)


# ---- the restatement against itself
def test_leaf_value_by_three_restatements():
    """200 mid-game positions of several shapes: the leaf value from the level flood, from the per-player distances and from
    the flood on Python ints is one number, for every live seat; contested cells, levels and empty leaves are counted alike"""
    seen = {"n": 0, "contested": 0, "values": set()}
    for N, P, B in ((5, 2, 40), (7, 3, 50), (9, 1, 20), (13, 4, 50), (33, 2, 20), (19, 8, 20)):
        st = M.positions(N, P, B, np.random.default_rng(N * 7 + P))
        for b in range(B):
            pos = M.pos_of(st, b)
            got = [T.leaf_areas(N, pos, m) for m in T.METHODS]
            assert got[0][0] == got[1][0] == got[2][0] and got[0][1:] == got[2][1:] and got[0][2] == got[1][2], (N, P, b, got)
            for seat in range(P):
                if pos.k[seat]:
                    continue
                vals = {T.leaf_value(N, pos, seat, 256, m) for m in T.METHODS}
                assert len(vals) == 1 and 0 <= min(vals) <= 512
                seen["values"] |= vals
            seen["n"] += 1
            seen["contested"] += got[0][2]
    assert seen["n"] == 200 and seen["contested"] >= 20 and len(seen["values"]) >= 30


@pytest.mark.parametrize("method", T.METHODS)
def test_search_is_the_same_by_every_restatement(method):
    st = M.positions(9, 3, 6, np.random.default_rng(2))
    want = T.tron_mcts_territory(st, 20, 100, 256, 3, 5, st.tcount, None, "avoid", 0.2)
    got = T.tron_mcts_territory(st, 20, 100, 256, 3, 5, st.tcount, None, "avoid", 0.2, method=method)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- hand-made answers
def _pos(d):
    """a Pos from a territory_ref hand board"""
    return M.Pos([int(x) for x in d["board"][0]], [int(x) for x in d["heads"][:, 0]], [int(x) for x in d["dirs"][:, 0]],
                 [int(x) for x in d["deaths"][:, 0]])


@pytest.mark.parametrize("method", T.METHODS)
@pytest.mark.parametrize("Vs", [1, 256, 1024])
def test_hand_made_leaf_values(method, Vs):
    # an even split: an empty 5x5 board, the players in the middle of the left and the right edge, facing each other -- nine
    # cells each, the middle column is reached by both at the same distance
    even = TV._pos(5, 2, np.zeros((5, 5), np.int8), [(0, 2), (4, 2)], [1, 3])
    count = T.new_count()
    assert T.leaf_areas(5, _pos(even), method)[0] == [9, 9]
    assert T.leaf_value(5, _pos(even), 0, Vs, method, count) == Vs == T.leaf_value(5, _pos(even), 1, Vs, method, count)
    assert count["contested"] == 2 and count["empty"] == 0
    # a sealed seat: player 0 walled in on all four sides, player 1 with the rest of the board
    walled = _pos(TV.hand_boards()["walled"])
    assert T.leaf_areas(5, walled, method)[0][0] == 0 and T.leaf_areas(5, walled, method)[0][1] > 0
    assert T.leaf_value(5, walled, 0, Vs, method) == 0 and T.leaf_value(5, walled, 1, Vs, method) == 2 * Vs
    # nobody has a free first cell: a full board
    full = TV._pos(3, 2, np.ones((3, 3), np.int8), [(0, 0), (2, 2)], [1, 3])
    count = T.new_count()
    assert T.leaf_value(3, _pos(full), 0, Vs, method, count) == Vs and count["empty"] == 1 and count["levels"] == 0
    # one player with room: everything it reaches is its own
    alone = _pos(TV.hand_boards()["spiral"])
    assert T.leaf_value(19, alone, 0, Vs, method) == 2 * Vs
    # a seat with 3 cells against 5: floor(2 V 3 / 8)
    cells = np.ones((5, 5), np.int8)
    cells[0, 1:4] = 0
    cells[4, 0:4] = 0
    cells[3, 0] = 0
    uneven = TV._pos(5, 2, cells, [(0, 0), (4, 4)], [1, 3])
    assert T.leaf_areas(5, _pos(uneven), method)[0] == [3, 5] and T.leaf_value(5, _pos(uneven), 0, Vs, method) == (6 * Vs) // 8


def test_corridor_three_one_step_values():
    """S = 3 expands the root's three actions once each; the avoid model without noise takes the other player one cell along
    its row (five cells left to it).  Forward: the seat keeps 3 cells of its corridor, floor(512 * 3 / 8) = 192.  Right: a
    closed-in cell, no first cell, 0.  Left: 2 cells, floor(512 * 2 / 7) = 146."""
    st = T.corridor_state()
    count = T.new_count()
    v, w, n, best = T.tron_mcts_territory(st, 3, 256, agent="avoid", noise=0.0, count=count)
    assert v.tolist() == [[1, 1, 1]] and w.tolist() == [[192, 0, 146]] and n.tolist() == [4] and best.tolist() == [0]
    assert count["flooded"] == 3 and count["closed"] == 0 and count["depth"] == 3 and count["empty"] == 0
    v, w, n, best = T.tron_mcts_territory(st, 3, 1000, agent="avoid", noise=0.0)
    assert w.tolist() == [[750, 0, 571]]


def test_nobody_has_a_first_cell():
    """forward takes both players onto their last free cell: an open leaf where a_s + a_o = 0, worth V; right and left hit
    a wall: closed, 0"""
    st = T.nowhere_state()
    count = T.new_count()
    v, w, n, best = T.tron_mcts_territory(st, 3, 300, agent="avoid", noise=0.0, count=count)
    assert v.tolist() == [[1, 1, 1]] and w.tolist() == [[300, 0, 0]] and best.tolist() == [0]
    assert count["empty"] == 1 and count["flooded"] == 1 and count["closed"] == 2


@pytest.mark.parametrize("agent", ["random", "avoid"])
def test_single_player(agent):
    """P = 1: every tree step is terminal, so every child is closed (2 V alive, 0 dead) and nothing is flooded"""
    from oracle import oracle as O
    st = O.TronState(5, 1, 1)
    st.board[0, 0], st.heads[0, 0], st.dirs[0, 0] = 1, 0, 1    # the corner (0, 0) heading east: left leaves the board
    count = T.new_count()
    v, w, n, best = T.tron_mcts_territory(st, 3, 7, cexp=0, agent=agent, count=count)
    assert v.tolist() == [[1, 1, 1]] and w.tolist() == [[14, 14, 0]] and n.tolist() == [4] and best.tolist() == [0]
    assert count["closed"] == 3 and count["flooded"] == 0


def test_search_leaves_the_pocket_alone():
    """Ahead a fork of two dead ends (eleven cells to Voronoi, six playable), to the right one corridor of nine; the other
    player's corridor lasts seven steps.  The one-ply territory-greedy action is forward (11 > 9).  The search sees the fork's
    value fall once a branch is entered and the corridor's rise to a win eight plies down: 64 simulations at exploration
    0.25 choose the corridor.  (Every corridor node has two fatal children, which a wider search keeps revisiting: at
    exploration 1.0 the same 64 simulations stay too shallow to reach the win.)"""
    st = T.pocket_state()
    N = st.N
    assert TV.greedy_action(N, st.board, st.heads, st.dirs, st.deaths, np.array([0]))[0] == 0
    area, _ = TV.territory(N, st.board, st.heads, st.dirs, st.deaths, np.array([0]), np.array([[0, 1, 2]]))
    assert area[0, :, 0].tolist() == [11, 9, 0]
    v, w, n, best = T.tron_mcts_territory(st, 64, 256, cexp=64, agent="avoid", noise=0.0)
    assert best[0] == 1 and v[0, 1] > v[0, 0] > v[0, 2] >= 1 and w[0, 2] == 0 and v[0].sum() == 64
    v3, w3, _, best3 = T.tron_mcts_territory(st, 3, 256, agent="avoid", noise=0.0)
    assert best3[0] == 0 and w3.tolist() == [[(512 * 10) // 16, (512 * 8) // 14, 0]]     # one ply deep it agrees with greedy


@pytest.mark.parametrize("S", [3, 64])
def test_step_rule_corners_by_hand(S):
    """The positions of tests/test_tron_mcts_host.py::test_step_rule_corners_by_hand with a flood at the leaves (avoid model,
    noise 0, V = 256).  Head-on, the seat first or second: forward is closed and lost.  After a turn into its own column the
    seat has the two cells left of that half-column, the model player in the dead end (2, 3) has none: floor(2 V 2 / 2) = 2 V,
    so S = 3 gives [0, 512, 512].  The bystander: three closed, won children, 2 V a visit.  The corner: forward and left
    leave the board; to the right the seat keeps five cells of its row against the other player's two: floor(512 * 5 / 7) =
    365."""
    seats = lambda s: np.array([s], np.int8)
    for seat in (0, 1):
        count = T.new_count()
        v, w, n, best = T.tron_mcts_territory(T.head_on_state(), S, seat=seats(seat), agent="avoid", noise=0.0, count=count)
        assert w[0, 0] == 0 and best[0] != 0 and v[0].sum() == S and v[0, 0] >= 1 and count["closed"] >= v[0, 0]
        assert count["head_on"] == 1                              # (one hit on a head: the expansion of the forward child)
        if S == 3:
            assert w.tolist() == [[0, 512, 512]] and n.tolist() == [4] and best.tolist() == [1] and count["flooded"] == 2
    count = T.new_count()
    v, w, n, best = T.tron_mcts_territory(T.head_on_state(3), S, seat=seats(2), agent="avoid", noise=0.0, count=count)
    assert n.tolist() == [4] and (w == 512 * v).all() and v[0].sum() == S and count["closed"] == S and count["flooded"] == 0
    assert count["head_on"] == 3
    v, w, n, best = T.tron_mcts_territory(T.corner_state(), S, agent="avoid", noise=0.0)
    assert w[0, 0] == 0 and w[0, 2] == 0 and best.tolist() == [1] and v[0].sum() == S
    if S == 3:
        assert w.tolist() == [[0, 365, 0]]


def test_skipped_positions_and_read_only_state():
    st = M.positions(7, 3, 6, np.random.default_rng(3))
    st.deaths[:, 0] = 0
    st.deaths[1, 1] = 3
    seat = np.array([0, 1, 3, -1, 0, 0])
    before = [x.copy() for x in (st.board, st.heads, st.dirs, st.deaths, st.tcount)]
    count = T.new_count()
    v, w, n, best = T.tron_mcts_territory(st, 12, 256, seat=seat, tcount=st.tcount, count=count)
    assert all(np.array_equal(a, b) for a, b in zip(before, (st.board, st.heads, st.dirs, st.deaths, st.tcount)))
    assert count["skipped"] >= 3 and (n[1:4] == 0).all() and (best[1:4] == -1).all() and (v[1:4] == 0).all() and (w[1:4] == 0).all()
    played = n > 0
    assert played[0] and (v[played].sum(axis=1) == 12).all() and (w <= 512 * v).all() and ((best >= 0) == played).all()
    assert count["closed"] + count["flooded"] == 12 * int(played.sum())
