"""The search valued by the caller's network (crl_ttt_puct_*) on the host: every CRL_EINVAL case of the five entries is
refused with its message before any device work, the tree's size, the Python wrappers' argument checks and `puct_quantize`,
and the plain-Python restatement of the header's contract (tests/puct_ref.py) -- the properties any such tree has, the case
table of the GPU test reaching the edges it names, and its strength against a tactical opponent next to flat Monte Carlo."""
import ctypes as C

import numpy as np
import pytest

from tests import mcts_ref as M
from tests import puct_cases as CASES
from tests import puct_ref as R
from tests.host_util import D, fake as _fake, lib as _lib, refused, tron_context, ttt_context
from tests.test_ttt_mcts_host import _flat_mc, _play, _state

ODD = C.c_void_p(72)                       # 8-byte aligned only


def _begin(lib, ctx, B=4, state=(D, D, D), S_cap=8, tree=D):
    return lib.crl_ttt_puct_begin(ctx, B, *state, S_cap, tree, None)


def _select(lib, ctx, B=4, tree=D, S_cap=8, cpuct=256, fpu=32768, rel_mod=2, outs=(D, D, D, D), leaf_occ=D, flags=0):
    return lib.crl_ttt_puct_select(ctx, B, tree, S_cap, cpuct, fpu, rel_mod, *outs, leaf_occ, flags, None)


def _backup(lib, ctx, B=4, tree=D, S_cap=8, prior=D, value=D, flags=0):
    return lib.crl_ttt_puct_backup(ctx, B, tree, S_cap, prior, value, flags, None)


def _root(lib, ctx, B=4, tree=D, S_cap=8, outs=(D,) * 6):
    return lib.crl_ttt_puct_root(ctx, B, tree, S_cap, *outs, None)


ENTRIES = (_begin, _select, _backup, _root)


def test_argument_checks_shared_by_the_entries():
    lib = _lib()
    with ttt_context() as h:
        for fn in ENTRIES:
            refused(lib, fn(lib, h, tree=None), b"NULL tree")
            refused(lib, fn(lib, h, tree=ODD), b"16-byte aligned")
            for B in (0, -1, (1 << 31) + 1):
                refused(lib, fn(lib, h, B=B), b"B=")
            for S_cap in (0, -1, 4096, 1 << 30):
                refused(lib, fn(lib, h, S_cap=S_cap), b"S_cap=")
            refused(lib, fn(lib, None), b"tictactoe")
    with tron_context() as tron:
        for fn in ENTRIES:
            refused(lib, fn(lib, tron), b"tictactoe")
        assert lib.crl_ttt_puct_tree_bytes(tron, 8) == -1 and b"tictactoe" in lib.crl_last_error()
    with ttt_context(1, 1, 2, 2, 3) as small:      # fewer cells than players
        for fn in ENTRIES:
            refused(lib, fn(lib, small), b"cells")


def test_argument_checks_of_each_entry():
    lib = _lib()
    with ttt_context() as h:
        for i in range(3):
            st = [D] * 3
            st[i] = None
            refused(lib, _begin(lib, h, state=tuple(st)), b"NULL state")
        for i in range(4):
            outs = [D] * 4
            outs[i] = None
            refused(lib, _select(lib, h, outs=tuple(outs)), b"NULL output")
        for cpuct in (65536, 0xFFFFFFFF):
            refused(lib, _select(lib, h, cpuct=cpuct), b"cpuct=")
        for fpu in (65537, 0xFFFFFFFF):
            refused(lib, _select(lib, h, fpu=fpu), b"fpu=")
        for rel_mod in (0, -1):
            refused(lib, _select(lib, h, rel_mod=rel_mod), b"rel_mod")
        for flags in (1, 8, 0x80000000):
            refused(lib, _select(lib, h, flags=flags), b"flags")
            refused(lib, _backup(lib, h, flags=flags), b"flags")
        # leaf_occ may be NULL, and the greatest cpuct, fpu and S_cap pass their checks: a later check (the flags) stops the call
        refused(lib, _select(lib, h, leaf_occ=None, cpuct=65535, fpu=65536, S_cap=4095, flags=1), b"flags")
        refused(lib, _backup(lib, h, prior=None), b"NULL input")
        refused(lib, _backup(lib, h, value=None), b"NULL input")
        for i in range(6):
            outs = [D] * 6
            outs[i] = None
            refused(lib, _root(lib, h, outs=tuple(outs)), b"NULL output")


@pytest.mark.parametrize("d, k, p", CASES.SHAPES, ids=CASES.SHAPE_IDS)
def test_tree_bytes(d, k, p):
    lib = _lib()
    d3 = (1,) * (3 - len(d)) + tuple(d)
    cells = d3[0] * d3[1] * d3[2]
    with ttt_context(*d3, k, p) as h:
        sizes = [lib.crl_ttt_puct_tree_bytes(h, s) for s in range(1, 4096)]
        assert all(n % 16 == 0 for n in sizes) and all(a < b for a, b in zip(sizes, sizes[1:]))     # monotone in S_cap
        assert all(n >= R.tree_bytes_floor(s, cells) for s, n in zip(range(1, 4096), sizes))
        assert sizes[-1] < 4 * R.tree_bytes_floor(4095, cells)
        for bad in (0, -5, 4096):
            assert lib.crl_ttt_puct_tree_bytes(h, bad) == -1 and b"S_cap=" in lib.crl_last_error()
    assert lib.crl_ttt_puct_tree_bytes(None, 8) == -1


def test_prototypes_and_abi():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    for name in ("tree_bytes", "begin", "select", "backup", "root"):
        assert "crl_ttt_puct_" + name in _native.PROTOTYPES


# ---- the Python wrappers refuse bad arguments before they reach the library
def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TTTBatch
    tb = _fake(TTTBatch, B=5, P=2, n_cells=9)
    for bad in (0, 4096, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            tb.puct_begin(bad)
        with pytest.raises(ValueError):
            tb.puct(lambda leaves: None, bad)
    for call in (tb.puct_select, tb.puct_root, lambda: tb.puct_backup(None, None)):
        with pytest.raises(ValueError, match="puct_begin"):
            call()
    tb._puct_cap, tb._puct_tree = 8, torch.zeros(4)
    for bad in (-0.5, 256.0, float("nan"), "1", True, None):
        with pytest.raises(ValueError):
            tb.puct_select(bad)
        with pytest.raises(ValueError):
            tb.puct(lambda leaves: None, 8, bad)
    for bad in (-0.1, 1.5, float("nan"), "x", None):
        with pytest.raises(ValueError):
            tb.puct_select(1.0, bad)
    for bad in (0, -1, 128, 1.0):
        with pytest.raises(ValueError):
            tb.puct_select(1.0, 0.5, bad)
    with pytest.raises(ValueError):
        tb.puct_select(out={"board": torch.zeros((5, 9), dtype=torch.int8)})
    with pytest.raises(ValueError):
        tb.puct_root(out={"visits": torch.zeros((5, 9), dtype=torch.int32)})
    good_p, good_v = torch.zeros((5, 9), dtype=torch.int16), torch.zeros((5, 2), dtype=torch.int32)
    for p, v in ((good_p.to(torch.int32), good_v), (good_p[:, :8].contiguous(), good_v), (good_p, good_v.to(torch.int64)),
                 (good_p, torch.zeros((5, 3), dtype=torch.int32)), (None, good_v), (good_p, None)):
        with pytest.raises(ValueError):
            tb.puct_backup(p, v)
    with pytest.raises(ValueError):
        tb.puct("not callable", 8)


def test_quantize():
    import torch
    from colosseumrl_amd.batched import TTTBatch
    pol = torch.tensor([[0.5, 0.25, 0.25, 0.0], [0.0, 0.0, 0.0, 0.0], [3.0, 1.0, float("nan"), 2.0], [1e-9, 2e-9, 0.0, 0.0]])
    val = torch.tensor([[0.0, 1.0], [0.5, 0.25], [2.0, -1.0], [float("nan"), 1.0]])
    prior, value = TTTBatch.puct_quantize(pol, val)
    assert prior.dtype == torch.int16 and value.dtype == torch.int32 and prior.shape == pol.shape and value.shape == val.shape
    u16 = prior.numpy().view(np.uint16)
    assert u16.tolist() == [[65535, 32768, 32768, 0], [0, 0, 0, 0], [65535, 21845, 0, 43690], [32768, 65535, 0, 0]]
    assert value.tolist() == [[0, 65536], [32768, 16384], [65536, 0], [32768, 65536]]


# ---- the restatement: the properties any such tree has
@pytest.mark.parametrize("d, k, p", CASES.SHAPES[:2], ids=CASES.SHAPE_IDS[:2])
def test_tree_invariants(d, k, p):
    st = M.positions(d, k, p, 16, np.random.default_rng(4))
    over = np.array([t.skipped for t in R.Search(st, 1).trees])
    assert over.sum() >= 4 and (~over).sum() >= 8
    for S in (1, 2, 9, 40):
        sr = R.Search(st, S)
        for s in range(S):
            leaves = sr.select()
            sr.backup(*R.evaluator(leaves["board"], leaves["mover"], p))
            for t in sr.trees:
                if t.skipped:
                    continue
                assert t.n[0] == t.sims == s + 1                                  # the root's n is the simulation count
                assert sum(t.n[u] for u in t.child[0] if u) == t.sims - 1         # the first simulation stops at the root
                assert all(w <= 65536 * n for n, w in zip(t.n, t.w)) and len(t.n) <= t.sims + 1
                assert all(t.expanded[u] == (t.n[u] > 0) for u in range(len(t.n)) if any(t.child[u]) or u == 0)
        out = sr.root()
        assert (out["nodes"][over] == 0).all() and (out["best"][over] == -1).all() and (out["visits"][over] == 0).all()
        assert (out["sims"][~over] == S).all() and (out["visits"][~over].sum(axis=1) == S - 1).all()
        assert ((out["best"][~over] >= 0) == (S > 1)).all()
        # a search that is over takes no more: select refuses, backup is a no-op
        count = R.new_count()
        sr.count = count
        leaves = sr.select()
        assert not leaves["pending"].any() and (leaves["mover"] == -1).all() and count["refused"] == (~over).sum()
        sr.backup(*R.evaluator(leaves["board"], leaves["mover"], p))
        again = sr.root()
        assert all(np.array_equal(out[key], again[key]) for key in out)


def test_select_twice_arrives_at_the_same_leaf():
    st = M.positions((3, 3), 3, 2, 6, np.random.default_rng(8), plant=False)
    a, b = R.Search(st, 30), R.Search(st, 30)
    for _ in range(30):
        la = a.select()
        b.select()
        lb = b.select()
        assert all(np.array_equal(la[key], lb[key]) for key in la)
        ev = R.evaluator(la["board"], la["mover"], 2)
        a.backup(*ev), b.backup(*ev)
    ra, rb = a.root(), b.root()
    assert all(np.array_equal(ra[key], rb[key]) for key in ra)


def test_forced_win_in_one_is_best_from_a_small_s_on():
    """Uniform priors, every value a draw's, fpu a draw's: children without a visit score alike and are tried in cell order,
    one simulation each, behind the simulation that expands the root.  The winning ply is a terminal child worth 65536 a
    visit, so it is `best` from the simulation that first tries it: by the larger w while every child has one visit, by its
    visits from then on."""
    # X (player 0, to move) completes the top row at cell 2, the lowest of the empty cells 2, 5, 6, 7, 8: tried in simulation 2
    low = _state((3, 3), 3, 2, [([0b000000011, 0b000011000], 0)])
    # X completes the bottom row at cell 8, the highest of the empty cells 0, 1, 2, 5, 8: tried in simulation 6
    high = _state((3, 3), 3, 2, [([0b011000000, 0b000011000], 0)])
    for st, cell, first in ((low, 2, 2), (high, 8, 6)):
        for S in range(1, 41):
            out, _ = R.run(st, S, mode="uniform")
            assert (out["best"][0] == cell) == (S >= first), (S, out["visits"][0])
        assert out["value"][0, cell] == 65536 * out["visits"][0, cell] and 2 * out["visits"][0, cell] > 40


def test_the_case_table_reaches_its_edges():
    """every row of the GPU test's case table, run on the restatement: the edge a row names shows in `count`"""
    for case in CASES.EDGE_CASES:
        count = R.new_count()
        st = CASES.edge_state(case)
        S, S_cap = case["S"], case.get("S_cap", case["S"])
        sr = R.Search(st, S_cap, count)
        for _ in range(S + case.get("extra", 0)):
            leaves = sr.select(case.get("cpuct", 256), case.get("fpu", 32768))
            sr.backup(*R.evaluator(leaves["board"], leaves["mover"], st.P, case.get("mode", "mix")))
        for key, least in case["reaches"].items():
            assert count[key] >= least, (case["id"], key, count)
    for shape, (d, k, p) in zip(CASES.SHAPE_IDS, CASES.SHAPES):
        count = R.new_count()
        st = CASES.positions(d, k, p, 130)
        R.run(st, CASES.simulations(d), count=count)
        skipped = sum(t.skipped for t in R.Search(st, 1).trees)
        assert skipped >= 2 and count["terminal"] > 0 and count["depth"] >= 3 and count["created"] > 130, (shape, count)


# ---- strength: PUCT with uniform priors and playout values against flat Monte Carlo at the same budget
def test_puct_beats_flat_monte_carlo_against_the_tactical_agent():
    """3x3, the learner at seat 1 against a noise-free tactical opponent that opens.  The PUCT learner: uniform priors, the
    value of a leaf the mean of 16 of mcts_ref's random playouts, S = 64, exploration 1.25, fpu 0.5 -- 1,024 playouts per move
    at the most.  The yardstick: test_ttt_mcts_host's flat Monte Carlo with 1,024 playouts per move, the same opponent draws.
    Condition: PUCT loses less often than flat Monte Carlo in the same run.
    Measured (100 games, seed 7, about 10 s): PUCT lost 9 of 100 (0.09), flat Monte Carlo 38 of 100 (0.38)."""
    game = M.Game((3, 3), 3, 2)
    games, seed, S, Rn = 100, 7, 64, 16

    def puct(g):
        def move(occ, c):
            t = R.Tree(game, occ, -1, 1)
            for s in range(S):
                leaf = t.select(S, R.cpuct_of(1.25), R.fpu_of(0.5))
                prior, value = [1] * 9, [0, 0]
                if leaf is not None:
                    pos, m = leaf
                    won = [M.playout(game, pos, m, seed, g, c + len(t.path) - 1, (s << 16) | r) for r in range(Rn)]
                    value = [(65536 * (2 * sum(w == (m + j) % 2 for w in won) + sum(w < 0 for w in won))) // (2 * Rn) for j in range(2)]
                t.backup(prior, value)
            return t.root()[5]
        return move

    def flat(g):
        return lambda occ, c: _flat_mc(game, occ, 1, S * Rn, seed, g, c)
    lost_puct = sum(_play(game, puct(g), g, seed) == 0 for g in range(games))
    lost_flat = sum(_play(game, flat(g), g, seed) == 0 for g in range(games))
    print("lost: puct %d / %d, flat MC %d / %d" % (lost_puct, games, lost_flat, games))
    assert lost_puct < lost_flat, (lost_puct, lost_flat)
