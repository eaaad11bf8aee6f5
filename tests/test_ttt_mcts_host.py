"""Batched Monte Carlo tree search (crl_ttt_mcts) on the host: the argument checks of the two C entries (every CRL_EINVAL
case is refused with its message before any device work), S_max per board, the argument checks of the Python wrappers, and
the plain-Python restatement of the header's contract (tests/mcts_ref.py) -- its own stepping and Philox held to the oracle,
the properties any such tree has, and its strength against a tactical opponent next to flat Monte Carlo."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mcts_ref as M
from tests import rng_ref as RNG
from tests.host_util import D, fake as _fake, lib as _lib, tron_context, ttt_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOARDS = [((1, 3, 3), 3, 2, 2519), ((1, 3, 5), 3, 3, 1723), ((3, 3, 3), 3, 4, 1056), ((1, 5, 5), 4, 3, 1128), ((1, 4, 8), 4, 2, 909)]


def _call(lib, ctx, B=4, state=None, S=8, Rn=4, cexp=256, outs=None, flags=0):
    occ, winner, to_move, tcount = state or (D, D, D, D)
    visits, value, nodes, best = outs or (D, D, D, D)
    return lib.crl_ttt_mcts(ctx, B, 1, 0, occ, winner, to_move, tcount, S, Rn, cexp, visits, value, nodes, best, flags, None)


def test_mcts_argument_checks():
    lib = _lib()
    with ttt_context() as h:
        for i in range(3):                 # occ, winner, to_move (tcount may be NULL)
            st = [D] * 4
            st[i] = None
            assert _call(lib, h, state=tuple(st)) == -1 and b"NULL state" in lib.crl_last_error()
        for i in range(4):
            outs = [D] * 4
            outs[i] = None
            assert _call(lib, h, outs=tuple(outs)) == -1 and b"NULL output" in lib.crl_last_error()
        for B in (0, -1, (1 << 31) + 1):
            assert _call(lib, h, B=B) == -1 and b"B=" in lib.crl_last_error()
        for S in (0, -1, 2520, 4096, 1 << 30):
            assert _call(lib, h, S=S) == -1 and b"S=" in lib.crl_last_error()
        for Rn in (0, -3, 1025, 65535):
            assert _call(lib, h, Rn=Rn) == -1 and b"R=" in lib.crl_last_error()
        for cexp in (65536, 0xFFFFFFFF):
            assert _call(lib, h, cexp=cexp) == -1 and b"cexp=" in lib.crl_last_error()
        for flags in (1, 8, 0x80000000):
            assert _call(lib, h, flags=flags) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, None) == -1 and b"tictactoe" in lib.crl_last_error()
        assert lib.crl_ttt_mcts_max_simulations(None) == -1 and b"tictactoe" in lib.crl_last_error()
    with tron_context() as tron:           # a context of another game
        assert _call(lib, tron) == -1 and b"tictactoe" in lib.crl_last_error()
        assert lib.crl_ttt_mcts_max_simulations(tron) == -1 and b"tictactoe" in lib.crl_last_error()
    with ttt_context(1, 1, 2, 2, 3) as small:   # fewer cells than players: refused as by crl_ttt_playout
        assert _call(lib, small) == -1 and b"cells" in lib.crl_last_error()


@pytest.mark.parametrize("d, k, p, s_max", BOARDS, ids=["3x3", "3x5", "3x3x3", "5x5", "4x8"])
def test_max_simulations(d, k, p, s_max):
    """S_max = min(4095, 65536 / (8 + 2 cells) - 1); S_max passes the check of S, S_max + 1 does not.  (The call with S_max
    is stopped by a later check -- the flags -- so that nothing is launched on the dummy pointers.)"""
    lib = _lib()
    cells = d[0] * d[1] * d[2]
    assert M.max_simulations(cells) == s_max == min(4095, 65536 // (8 + 2 * cells) - 1)
    assert (s_max + 1) * (8 + 2 * cells) <= 65536 < (s_max + 2) * (8 + 2 * cells) or s_max == 4095
    with ttt_context(*d, k, p) as h:
        assert lib.crl_ttt_mcts_max_simulations(h) == s_max
        assert _call(lib, h, S=s_max, flags=1) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, h, S=s_max + 1, flags=1) == -1 and b"S=" in lib.crl_last_error()


def test_max_simulations_small_board():
    lib = _lib()                           # the 12 bits of s in the counter word bound S on small boards
    with ttt_context(1, 1, 3, 2, 2) as h:
        assert lib.crl_ttt_mcts_max_simulations(h) == 4095 == M.max_simulations(3)


def test_mcts_prototypes_and_tag():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    assert "crl_ttt_mcts" in _native.PROTOTYPES and "crl_ttt_mcts_max_simulations" in _native.PROTOTYPES
    common = open(os.path.join(ROOT, "colosseumrl_amd", "csrc", "crl_common.hpp")).read()
    tags = re.findall(r"#define\s+(CRL_TAG_\w+)\s+(0x[0-9a-fA-F]+)u", common)
    assert ("CRL_TAG_TTT_MCTS", RNG.tag_hex("CRL_TAG_TTT_MCTS")) in tags
    values = [int(v, 16) for _, v in tags]
    assert len(set(values)) == len(values) and values.count(M.TAG_TTT_MCTS) == 1     # used nowhere else


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TTTBatch, _exploration
    tb = _fake(TTTBatch, B=5, P=2, n_cells=9)
    tb.__dict__["mcts_max_simulations"] = 2519
    for fn in (tb.mcts, tb.mcts_action):
        for bad in (0, 2520, -1, 2.0, True, None):
            with pytest.raises(ValueError):
                fn(bad)
        for bad in (0, 1025, 16.0, False):
            with pytest.raises(ValueError):
                fn(8, bad)
        for bad in (-0.5, 256.0, float("nan"), "1", True, None):
            with pytest.raises(ValueError):
                fn(8, 16, 0, bad)
    i32 = torch.int32
    good = {"visits": torch.zeros((5, 9), dtype=i32), "value": torch.zeros((5, 9), dtype=i32),
            "nodes": torch.zeros((5,), dtype=i32), "best": torch.zeros((5,), dtype=i32)}
    for key, wrong in (("visits", torch.zeros((5, 8), dtype=i32)), ("value", torch.zeros((5, 9), dtype=torch.int64)),
                       ("nodes", torch.zeros((4,), dtype=i32)), ("best", torch.zeros((5,), dtype=torch.int64))):
        with pytest.raises(ValueError):
            tb.mcts(8, out=dict(good, **{key: wrong}))
        with pytest.raises(ValueError):
            tb.mcts(8, out={k: v for k, v in good.items() if k != key})
    assert [_exploration("e", v) for v in (0, 1, 1.0, 0.5, 1.4142, 65535 / 256)] == [0, 256, 256, 128, 362, 65535]
    assert all(M.cexp_of(v) == _exploration("e", v) for v in (0.0, 0.3, 1.0, 2.5, 100.0))


# ---- the restatement: its parts
def test_lg():
    assert all(M.lg(1 << k) == 256 * k for k in range(32))
    vals = [M.lg(n) for n in range(1, 70000)]
    assert all(a <= b for a, b in zip(vals, vals[1:]))
    assert M.lg(3) == 256 + 128 and M.lg(5) == 512 + 64 and M.lg(4095) == 256 * 11 + 255 and M.lg(511) == 256 * 8 + 255
    assert M.lg(0x1FF00) == M.lg(0x1FFFF) == 256 * 16 + 255     # only the 8 bits below the leading one count


def test_score():
    # exploit alone: all playouts won = 65536, all drawn = 32768
    assert M.score(7, 3, 2 * 3 * 16, 16, 0) == 65536 and M.score(7, 3, 3 * 16, 16, 0) == 32768 and M.score(9, 2, 0, 5, 0) == 0
    # n_v = 4, n_u = 1: X = 512 << 24, isqrt = 92681, cexp = 256 adds isqrt itself = sqrt(2) * 65536
    assert M.score(4, 1, 0, 1, 256) == 92681 and M.score(4, 1, 0, 1, 512) == 2 * 92681 and M.score(4, 1, 0, 1, 128) == 92681 // 2
    assert M.score(1, 1, 2, 1, 65535) == 65536                   # lg(1) = 0: no exploration term at all
    assert M.score(4095, 1, 2 * 1024, 1024, 65535) < 1 << 26     # the greatest score there is


def test_fast_stepping_and_philox_match_the_oracle():
    """the restatement's own masks against oracle.ttt_step on whole random games, its Philox against oracle.philox4x32"""
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    for dims, K, P in [((3, 3), 3, 2), ((3, 5), 3, 3), ((3, 3, 3), 3, 4), ((5, 5), 4, 3), ((4, 8), 4, 2)]:
        game = M.Game(dims, K, P)
        for _ in range(40):
            st = O.TTTState(dims, K, P, 1)
            occ, tm, term = [0] * P, 0, False
            while not term:
                cell = int(rng.choice(M._empty_cells(game, occ)))
                term, ws = game.step(occ, tm, cell)
                _, t2, w2 = O.ttt_step(st, np.array([cell], np.int8))
                assert (bool(t2[0]), int(w2[0])) == (term, ws) and [int(x) for x in st.occ[:, 0]] == occ
                tm = (tm + 1) % P
                assert int(st.to_move[0]) == tm
    for _ in range(200):
        args = [int(x) for x in rng.integers(0, 2 ** 32, size=6)]
        assert M.philox(*args) == tuple(int(x) for x in O.philox4x32(args[:4], args[4:]))


def _state(dims, K, P, positions):
    from oracle import oracle as O
    st = O.TTTState(dims, K, P, len(positions))
    for b, (occ, tm) in enumerate(positions):
        st.occ[:, b], st.to_move[b] = occ, tm
    return st


def test_search_through_the_oracle_itself():
    """the same trees whether the plies and draws are the restatement's own or the oracle's"""
    rng = np.random.default_rng(2)
    st = M.positions((3, 3), 3, 2, 8, rng)
    for S, Rn, cexp in ((12, 3, 256), (30, 1, 0)):
        fast = M.ttt_mcts(st, S, Rn, cexp, seed=9, first_env_id=4, tcount=st.tcount)
        slow = M.ttt_mcts(st, S, Rn, cexp, seed=9, first_env_id=4, tcount=st.tcount, stepper="oracle")
        assert all(np.array_equal(a, b) for a, b in zip(fast, slow))


def test_tree_properties():
    rng = np.random.default_rng(3)
    for dims, K, P in [((3, 3), 3, 2), ((3, 5), 3, 3)]:
        st = M.positions(dims, K, P, 24, rng)
        before = (st.occ.copy(), st.winner.copy(), st.to_move.copy(), st.tcount.copy())
        n = st.n_cells
        empties = np.array([n - bin(int(np.bitwise_or.reduce(st.occ[:, b]))).count("1") for b in range(st.B)])
        over = (st.winner >= 0) | (empties == 0) | (st.to_move < 0) | (st.to_move >= P)
        assert over.sum() >= 4 and (~over).sum() >= 12
        for S in (1, 7, 40):
            visits, value, nodes, best = M.ttt_mcts(st, S, 4, 256, seed=1, tcount=st.tcount)
            assert all(np.array_equal(a, b) for a, b in zip(before, (st.occ, st.winner, st.to_move, st.tcount)))   # read only
            assert (visits[over] == 0).all() and (value[over] == 0).all() and (nodes[over] == 0).all() and (best[over] == -1).all()
            run = ~over
            assert (visits[run].sum(axis=1) == S).all() and (nodes[run] <= S + 1).all() and (nodes[run] >= 2).all()
            assert (value[run] <= 2 * 4 * visits[run]).all()
            for b in np.flatnonzero(run):
                occ = int(np.bitwise_or.reduce(st.occ[:, b]))
                assert all(visits[b, c] == 0 for c in range(n) if (occ >> c) & 1)            # children at empty cells only
                assert visits[b, best[b]] == visits[b].max() and not (occ >> int(best[b])) & 1
                top = [c for c in range(n) if visits[b, c] == visits[b].max() and not (occ >> c) & 1]
                assert best[b] == min(c for c in top if value[b, c] == max(value[b, t] for t in top))
                if S <= empties[b]:                                                           # expansion only, lowest cells first
                    free = [c for c in range(n) if not (occ >> c) & 1]
                    assert [c for c in range(n) if visits[b, c]] == free[:S] and nodes[b] == S + 1


def test_one_visit_per_child_when_simulations_equal_empty_cells():
    for occ, tm in [([0, 0], 0), ([0b000010000, 0], 1), ([0b100000001, 0b000010000], 1), ([0b010001100, 0b001100010], 0)]:
        st = _state((3, 3), 3, 2, [(occ, tm)])
        S = 9 - bin(occ[0] | occ[1]).count("1")
        visits, value, nodes, best = M.ttt_mcts(st, S, 8, 256, seed=2)
        assert [int(v) for v in visits[0]] == [0 if ((occ[0] | occ[1]) >> c) & 1 else 1 for c in range(9)] and nodes[0] == S + 1


def test_terminal_leaves_and_the_tie_rules():
    # X (player 0, to move) completes the top row at cell 2: that child is a terminal node, every visit worth 2 R
    st = _state((3, 3), 3, 2, [([0b000000011, 0b000011000], 0)])
    visits, value, nodes, best = M.ttt_mcts(st, 40, 5, 256, seed=3)
    assert value[0, 2] == 2 * 5 * visits[0, 2] and best[0] == 2 and visits[0, 2] == visits[0].max() and nodes[0] <= 41
    # pure exploitation keeps revisiting the won child once every cell has been tried
    visits, value, nodes, best = M.ttt_mcts(st, 40, 5, 0, seed=3)
    assert visits[0, 2] == 40 - 4 and nodes[0] == 6                       # (5 empty cells: 2, 5, 6, 7, 8)
    # one empty cell, S = 3: the one child is terminal (a draw) and is visited every time
    st = _state((3, 3), 3, 2, [([0b101001110 & ~0b10, 0b010110001], 0)])
    assert bin(int(st.occ[0, 0]) | int(st.occ[1, 0])).count("1") == 8
    visits, value, nodes, best = M.ttt_mcts(st, 3, 7, 256)
    assert visits[0].sum() == 3 and nodes[0] == 2 and best[0] == 1 and value[0, 1] in (3 * 7, 3 * 14)


# ---- strength: the search against flat Monte Carlo at the same budget, seat 1, a noise-free tactical opponent
_LINES = [0b000000111, 0b000111000, 0b111000000, 0b001001001, 0b010010010, 0b100100100, 0b100010001, 0b001010100]


def _winning(mine, empty):
    return [c for c in empty if any((mine | 1 << c) & ln == ln for ln in _LINES)]


def _tactical(occ, me, rng):
    empty = [c for c in range(9) if not ((occ[0] | occ[1]) >> c) & 1]
    return int(rng.choice(_winning(occ[me], empty) or _winning(occ[1 - me], empty) or empty))


def _flat_mc(game, occ, tm, budget, seed, g, c):
    """the lowest cell of the greatest 2 wins + draws over ceil(budget / cells) random playouts behind each empty cell"""
    empty = M._empty_cells(game, occ)
    Rn = -(-budget // len(empty))
    best, best_v = -1, -1
    for cell in empty:
        o = list(occ)
        term, ws = game.step(o, tm, cell)
        if term:
            v = Rn * (2 if ws == tm else 1)
        else:
            v = 0
            for r in range(Rn):
                ws = M.playout(game, o, (tm + 1) % game.P, seed, g, c + 1, (cell << 16) | r, tag=RNG.CRL_TAG_TTT_PLAYOUT)
                v += 2 if ws == tm else (1 if ws < 0 else 0)
        if v > best_v:
            best, best_v = cell, v
    return best


def _play(game, learner, g, seed):
    """one game, the tactical agent at seat 0, `learner(occ, c)` at seat 1: the winner or -1"""
    rng = np.random.default_rng([seed, g])
    occ, tm, c = [0, 0], 0, 0
    while True:
        cell = _tactical(occ, 0, rng) if tm == 0 else learner(occ, c)
        term, ws = game.step(occ, tm, cell)
        if term:
            return ws
        tm, c = 1 - tm, c + 1


def test_search_beats_flat_monte_carlo_against_the_tactical_agent():
    """3x3, the learner at seat 1 against a noise-free tactical opponent that opens: a search of 128 simulations x 16 playouts
    (exploration 1.0) against flat Monte Carlo with the same 2,048 playouts per move, on the restatement alone.  The same
    opponent draws serve both learners.  Condition: the search loses at most half as often as flat Monte Carlo.
    Measured (100 games, seed 7, about 25 s): the search lost 4 of 100 (0.04), flat Monte Carlo 37 of 100 (0.37)."""
    game = M.Game((3, 3), 3, 2)
    games, seed = 100, 7

    def search(g):
        return lambda occ, c: M.search(game, occ, 1, 128, 16, 256, seed, g, c)[3]

    def flat(g):
        return lambda occ, c: _flat_mc(game, occ, 1, 2048, seed, g, c)
    lost_search = sum(_play(game, search(g), g, seed) == 0 for g in range(games))
    lost_flat = sum(_play(game, flat(g), g, seed) == 0 for g in range(games))
    print("lost: search %d / %d, flat MC %d / %d" % (lost_search, games, lost_flat, games))
    assert lost_flat > 0 and 2 * lost_search <= lost_flat, (lost_search, lost_flat)
