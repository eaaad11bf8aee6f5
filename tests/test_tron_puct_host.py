"""The Tron search valued by the caller's network (crl_tron_puct_*) on the host: every CRL_EINVAL case of the five entries is
refused with its message before any device work, the tree's size, the Python wrappers' argument checks and `puct_quantize`,
and the plain-Python restatement of the header's contract (tests/tron_puct_ref.py) -- the properties any such tree has, its
leaf positions against a replay with oracle.tron_step, the deep-path row closing where the GPU test says it does, and the
case table of the GPU test reaching the edges it names: every player count among the shapes with every player seated, the
hand-laid boards below 16 cells, the boards on either side of every change of `select`'s wave count, the capacity rows'
tree sizes, and every crash kind of the step above a pending leaf under both models."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import tron_mcts_ref as TM
from tests import tron_puct_cases as CASES
from tests import tron_puct_ref as R
from tests.host_util import D, fake as _fake, lib as _lib, refused, tron_context, ttt_context
from tests.rng_ref import M32, threshold

ODD = C.c_void_p(72)                       # 8-byte aligned only
# the tests of the restatement alone belong to the entries too: without them in the library this module does not import
assert _lib().crl_tron_puct_tree_bytes is not None
_D = C.c_double


def _begin(lib, ctx, B=4, state=(D, D, D, D), tcount=D, seat=D, S_cap=8, noise=0.1, flags=0, tree=D):
    return lib.crl_tron_puct_begin(ctx, B, 0, 0, *state, tcount, seat, S_cap, _D(noise), flags, tree, None)


def _select(lib, ctx, B=4, tree=D, S_cap=8, cpuct=256, fpu=32768, outs=(D,) * 6, leaf=(D,) * 4, flags=0):
    return lib.crl_tron_puct_select(ctx, B, tree, S_cap, cpuct, fpu, *outs, *leaf, flags, None)


def _backup(lib, ctx, B=4, tree=D, S_cap=8, prior=D, value=D, flags=0):
    return lib.crl_tron_puct_backup(ctx, B, tree, S_cap, prior, value, flags, None)


def _root(lib, ctx, B=4, tree=D, S_cap=8, outs=(D,) * 6):
    return lib.crl_tron_puct_root(ctx, B, tree, S_cap, *outs, None)


ENTRIES = (_begin, _select, _backup, _root)


def test_argument_checks_shared_by_the_entries():
    lib = _lib()
    with tron_context() as h:
        for fn in ENTRIES:
            refused(lib, fn(lib, h, tree=None), b"NULL tree")
            refused(lib, fn(lib, h, tree=ODD), b"16-byte aligned")
            for B in (0, -1, (1 << 31) + 1):
                refused(lib, fn(lib, h, B=B), b"B=")
            for S_cap in (0, -1, 4096, 1 << 30):
                refused(lib, fn(lib, h, S_cap=S_cap), b"S_cap=")
            refused(lib, fn(lib, None), b"not a tron context")
    with ttt_context() as ttt:
        for fn in ENTRIES:
            refused(lib, fn(lib, ttt), b"not a tron context")
        assert lib.crl_tron_puct_tree_bytes(ttt, 8) == -1 and b"not a tron context" in lib.crl_last_error()


def test_argument_checks_of_each_entry():
    lib = _lib()
    with tron_context() as h:
        for i in range(4):
            st = [D] * 4
            st[i] = None
            refused(lib, _begin(lib, h, state=tuple(st)), b"NULL state")
        for noise in (-0.01, 1.01, float("nan"), float("inf")):
            refused(lib, _begin(lib, h, noise=noise), b"noise=")
        for flags in (2, 3, 8, 0x80000000):
            refused(lib, _begin(lib, h, flags=flags), b"flags")
        # tcount and seat may be NULL, and CRL_PLAYOUT_AVOID and the noise bounds pass: a later check (the tree) stops the call
        for noise in (0.0, 1.0):
            refused(lib, _begin(lib, h, tcount=None, seat=None, noise=noise, flags=1, tree=ODD), b"16-byte aligned")
        for i in range(6):
            outs = [D] * 6
            outs[i] = None
            refused(lib, _select(lib, h, outs=tuple(outs)), b"NULL output")
        for gone in ((0,), (1,), (2,), (3,), (0, 1), (1, 2, 3), (0, 3)):
            leaf = [None if i in gone else D for i in range(4)]
            refused(lib, _select(lib, h, leaf=tuple(leaf)), b"all NULL or none")
        for cpuct in (65536, 0xFFFFFFFF):
            refused(lib, _select(lib, h, cpuct=cpuct), b"cpuct=")
        for fpu in (65537, 0xFFFFFFFF):
            refused(lib, _select(lib, h, fpu=fpu), b"fpu=")
        for flags in (1, 8, 0x80000000):
            refused(lib, _select(lib, h, flags=flags), b"flags")
            refused(lib, _backup(lib, h, flags=flags), b"flags")
        # the leaf set may be NULL as a whole, and the greatest cpuct, fpu and S_cap pass their checks: the flags stop the call
        refused(lib, _select(lib, h, leaf=(None,) * 4, cpuct=65535, fpu=65536, S_cap=4095, flags=1), b"flags")
        refused(lib, _backup(lib, h, prior=None), b"NULL input")
        refused(lib, _backup(lib, h, value=None), b"NULL input")
        for i in range(6):
            outs = [D] * 6
            outs[i] = None
            refused(lib, _root(lib, h, outs=tuple(outs)), b"NULL output")


@pytest.mark.parametrize("N, P", [(2, 1), (5, 2), (13, 4), (19, 4), (20, 4), (67, 2), (181, 8)])
def test_tree_bytes(N, P):
    lib = _lib()
    heads = [i * (N + 1) % (N * N) for i in range(P)] if N > 2 else [0]
    with tron_context(N, P, heads[:P], [0] * P) as h:
        sizes = [lib.crl_tron_puct_tree_bytes(h, s) for s in range(1, 4096)]
        assert all(n % 16 == 0 for n in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
        assert all(a < b for a, b in zip(sizes, sizes[8:]))                         # grows with S_cap (22 bytes a node, in 16s)
        assert all(n >= R.tree_bytes_floor(s, N) for s, n in zip(range(1, 4096), sizes))
        assert sizes[-1] < 2 * R.tree_bytes_floor(4095, N)
        for bad in (0, -5, 4096):
            assert lib.crl_tron_puct_tree_bytes(h, bad) == -1 and b"S_cap=" in lib.crl_last_error()
        # every board a context can have fits the LDS byte copy: the shared checks pass and a later one stops the call
        refused(lib, _select(lib, h, flags=1), b"flags")
    assert lib.crl_tron_puct_tree_bytes(None, 8) == -1


def test_prototypes_and_abi():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    for name in ("tree_bytes", "begin", "select", "backup", "root"):
        assert "crl_tron_puct_" + name in _native.PROTOTYPES


# ---- the Python wrappers refuse bad arguments before they reach the library
def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TronBatch
    tb = _fake(TronBatch, B=5, P=2, N=5)
    assert TronBatch.PUCT_MAX_CAPACITY == 4095
    for bad in (0, 4096, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            tb.puct_begin(bad)
        with pytest.raises(ValueError):
            tb.puct(lambda leaves: None, bad)
    for kw in ({"agent": "greedy"}, {"agent": None}, {"noise": -0.1}, {"noise": 1.5}, {"noise": float("nan")}, {"noise": "x"},
               {"seat": [0] * 5}, {"seat": torch.zeros(5, dtype=torch.int32)}, {"seat": torch.zeros(4, dtype=torch.int8)}):
        with pytest.raises(ValueError):
            tb.puct_begin(8, **kw)
        with pytest.raises(ValueError):
            tb.puct(lambda leaves: None, 8, **kw)
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
        with pytest.raises(ValueError):
            tb.puct(lambda leaves: None, 8, 1.0, bad)
    with pytest.raises(ValueError):
        tb.puct_select(out={"obs_board": torch.zeros((5, 25), dtype=torch.int8)})
    full = {k: torch.zeros(shape, dtype=dt) for k, (dt, shape) in tb._puct_select_spec().items()}
    for key, wrong in (("obs_board", torch.zeros((5, 24), dtype=torch.int8)), ("obs_heads", torch.zeros((2, 5), dtype=torch.int8)),
                       ("depth", torch.zeros((5,), dtype=torch.int64)), ("leaf_deaths", torch.zeros((5, 2), dtype=torch.int8))):
        with pytest.raises(ValueError):
            tb.puct_select(out=dict(full, **{key: wrong}))
    with pytest.raises(ValueError):
        tb.puct_root(out={"visits": torch.zeros((5, 3), dtype=torch.int32)})
    good_p, good_v = torch.zeros((5, 3), dtype=torch.int16), torch.zeros((5,), dtype=torch.int32)
    for p, v in ((good_p.to(torch.int32), good_v), (good_p[:, :2].contiguous(), good_v), (good_p, good_v.to(torch.int64)),
                 (good_p, torch.zeros((5, 2), dtype=torch.int32)), (None, good_v), (good_p, None)):
        with pytest.raises(ValueError):
            tb.puct_backup(p, v)
    with pytest.raises(ValueError):
        tb.puct("not callable", 8)
    with pytest.raises(ValueError):
        tb.puct_action("not callable", 8)


def test_quantize():
    import torch
    from colosseumrl_amd.batched import TronBatch
    pol = torch.tensor([[0.5, 0.25, 0.25], [0.0, 0.0, 0.0], [3.0, float("nan"), 2.0], [1e-9, 2e-9, 0.0]])
    val = torch.tensor([0.0, 0.25, 2.0, float("nan")])
    prior, value = TronBatch.puct_quantize(pol, val)
    assert prior.dtype == torch.int16 and value.dtype == torch.int32 and prior.shape == pol.shape and value.shape == val.shape
    u16 = prior.numpy().view(np.uint16)
    assert u16.tolist() == [[65535, 32768, 32768], [0, 0, 0], [65535, 0, 43690], [32768, 65535, 0]]
    assert value.tolist() == [0, 16384, 65536, 32768]


# ---- the restatement: the properties any such tree has
@pytest.mark.parametrize("shape", [0, 1, 4], ids=[CASES.SHAPE_IDS[i] for i in (0, 1, 4)])
def test_tree_invariants(shape):
    N, P, agent = CASES.SHAPES[shape]
    st, seat = CASES.state(N, P, 16), CASES.seats(P, 16)
    over = np.array([t.skipped for t in R.Search(st, 1, seat=seat).trees])
    assert over.sum() >= 2 and (~over).sum() >= 8
    for S in (1, 2, 9, 40):
        sr = R.Search(st, S, seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID, seat=seat, agent=agent, noise=CASES.NOISE)
        for s in range(S):
            leaves = sr.select()
            sr.backup(*R.evaluator(leaves["obs_board"], leaves["obs_heads"], leaves["obs_dirs"]))
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
        assert not leaves["pending"].any() and not leaves["obs_board"].any() and count["refused"] == (~over).sum()
        sr.backup(*R.evaluator(leaves["obs_board"], leaves["obs_heads"], leaves["obs_dirs"]))
        again = sr.root()
        assert all(np.array_equal(out[key], again[key]) for key in out)


def _replay(st, b, seat, edges, agent, noise, seed, g, tc):
    """the position behind `edges` from row b of `st`: the model's actions from tron_mcts_ref, the steps by oracle.tron_step"""
    one = O.TronState(st.N, st.P, 1)
    one.board[0], one.heads[:, 0], one.dirs[:, 0], one.deaths[:, 0] = st.board[b], st.heads[:, b], st.dirs[:, b], st.deaths[:, b]
    for k, e in enumerate(edges):
        act = TM.model_actions(st.N, TM.pos_of(one, 0), agent, threshold(noise), seed & M32, (seed >> 32) & M32, g & M32, (tc + k) & M32,
                               TM.TREE_STEP)
        act[seat] = (0, 1, -1)[e]
        O.tron_step(one, np.array(act, np.int8).reshape(st.P, 1))
    return one


def _replayed(st, seat, agent, noise, S, cpuct=256, count=None):
    """S simulations on the restatement, every pending leaf (the leaf_* position and the observation) against a replay of its
    edges with oracle.tron_step: the number of such leaves below the root"""
    sr = R.Search(st, S, seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID, seat=seat, agent=agent, noise=noise, count=count)
    checked = 0
    for s in range(S):
        leaves = sr.select(cpuct)
        for b, t in enumerate(sr.trees):
            if not leaves["pending"][b]:
                continue
            edges = t.edges()
            assert leaves["depth"][b] == len(edges)
            one = _replay(st, b, t.seat, edges, agent, noise, CASES.SEED, CASES.FIRST_ENV_ID + b, int(st.tcount[b]))
            assert np.array_equal(one.board[0], leaves["leaf_board"][b]) and np.array_equal(one.heads[:, 0], leaves["leaf_heads"][:, b])
            assert np.array_equal(one.dirs[:, 0], leaves["leaf_dirs"][:, b]) and np.array_equal(one.deaths[:, 0], leaves["leaf_deaths"][:, b])
            ob, oh, od, ok = O.tron_observe(one, np.array([t.seat], np.int8))
            assert np.array_equal(ob[0], leaves["obs_board"][b]) and np.array_equal(oh[:, 0], leaves["obs_heads"][:, b])
            assert np.array_equal(od[:, 0], leaves["obs_dirs"][:, b]) and np.array_equal(ok[:, 0], leaves["obs_deaths"][:, b])
            checked += len(edges) > 0
        sr.backup(*R.evaluator(leaves["obs_board"], leaves["obs_heads"], leaves["obs_dirs"]))
    return checked


@pytest.mark.parametrize("shape", [1, 3], ids=[CASES.SHAPE_IDS[i] for i in (1, 3)])
def test_leaf_positions_equal_a_replay_with_the_oracle_step(shape):
    N, P, agent = CASES.SHAPES[shape]
    checked = _replayed(CASES.state(N, P, 12), CASES.seats(P, 12), agent, CASES.NOISE, 25)
    assert checked >= 12                                                         # (a leaf below the root per row, on average, at the least)


def test_select_twice_arrives_at_the_same_leaf():
    N, P, agent = CASES.SHAPES[0]
    st, seat = CASES.state(N, P, 6), CASES.seats(P, 6)
    a, b = R.Search(st, 30, seat=seat, agent=agent), R.Search(st, 30, seat=seat, agent=agent)
    for _ in range(30):
        la = a.select()
        b.select()
        lb = b.select()
        assert all(np.array_equal(la[key], lb[key]) for key in la)
        ev = R.evaluator(la["obs_board"], la["obs_heads"], la["obs_dirs"])
        a.backup(*ev), b.backup(*ev)
    ra, rb = a.root(), b.root()
    assert all(np.array_equal(ra[key], rb[key]) for key in ra)


def test_the_deep_row_goes_one_ply_deeper_per_simulation_and_closes_at_depth_67():
    """the GPU test's path of more than 64 nodes, on the CPU: tree_step along the top row of the 67x67 board closes exactly at
    depth 67 under the avoid model at noise 0 (the random model would close player 1, and the tree, at once)"""
    st, row = CASES.deep_state(), CASES.DEEP
    pos = TM.pos_of(st, 0)
    for k in range(row["closes_at"]):
        assert not TM.is_closed(pos, 0), k
        TM.tree_step(67, pos, 0, 0, "avoid", threshold(0.0), 0, 0, 0, k)
    assert TM.is_closed(pos, 0) and pos.k[0] == 1 and pos.k[1] == 0            # the seat ran off the board; player 1 lives
    count = R.new_count()
    out, seen = R.run(st, row["S"], cpuct=row["cpuct"], fpu=row["fpu"], mode=row["mode"], count=count, record=True,
                      agent=row["agent"], noise=row["noise"], use_tcount=False)
    assert [int(s["depth"][0]) for s in seen[:67]] == list(range(67)) and all(s["pending"][0] for s in seen[:67])
    assert not any(s["pending"][0] for s in seen[67:])                          # the terminal leaf at depth 67, three times
    assert count["depth"] == 67 and count["terminal"] == 3 and out["nodes"][0] == 68 and out["visits"][0].tolist() == [69, 0, 0]


def test_the_case_table_reaches_its_edges():
    """every row of the GPU test's case table, run on the restatement: the edge a row names shows in `count`"""
    for case in CASES.EDGE_CASES:
        count = R.new_count()
        st, seat, agent = CASES.edge_state(case)
        S, S_cap = case["S"], case.get("S_cap", case["S"])
        sr = R.Search(st, S_cap, seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID, seat=seat, agent=agent, noise=CASES.NOISE,
                      count=count)
        for _ in range(S + case.get("extra", 0)):
            leaves = sr.select(case.get("cpuct", 256), case.get("fpu", 32768))
            sr.backup(*R.evaluator(leaves["obs_board"], leaves["obs_heads"], leaves["obs_dirs"], case.get("mode", "mix")))
        for key, least in case["reaches"].items():
            assert count[key] >= least, (case["id"], key, count)
    for index, (shape, (N, P, agent)) in enumerate(zip(CASES.SHAPE_IDS, CASES.SHAPES)):
        count = R.new_count()
        st, seat = CASES.state(N, P, 130), CASES.shape_seats(index, 130)
        if index < CASES.N_FIRST_SHAPES:
            assert np.array_equal(seat, CASES.seats(P, 130))                      # (the first seven shapes keep their seats)
        else:                                                                    # every player is the seat of a live tree
            assert {t.seat for t in R.Search(st, 1, seat=seat).trees if not t.skipped} == set(range(P)), shape
        R.run(st, CASES.S_MAIN, count=count, seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID, seat=seat, agent=agent,
              noise=CASES.NOISE)
        skipped = sum(t.skipped for t in R.Search(st, 1, seat=seat).trees)
        assert skipped >= 2 and count["terminal"] > 0 and count["created"] > 130, (shape, count)
        assert count["depth"] >= (1 if P == 1 else 3), (shape, count)
        assert 2 ** 32 - 3 in st.tcount.tolist()                                 # the counter wrap is among the rows


def test_every_player_count_is_among_the_shapes():
    """the eight template instances of `begin` and `select` all run, the odd player counts under both models, and the
    smallest start-layout board with rows of one 16-byte chunk"""
    assert {P for N, P, agent in CASES.SHAPES} == set(range(1, 9))
    for P in (3, 5, 6, 7):
        assert {agent for N, p, agent in CASES.SHAPES if p == P} == {"random", "avoid"}
        assert all((N * N) % 16 for N, p, agent in CASES.SHAPES if p == P and N > 4)     # planes off the 16-byte grid
    assert (4, 2, "avoid") in CASES.SHAPES and (4, 3, "random") in CASES.SHAPES
    assert len(CASES.SHAPE_IDS) == len(CASES.SHAPES) == len(set(CASES.SHAPE_IDS))
    assert CASES.SHAPES[:7] == [(5, 2, "random"), (13, 4, "avoid"), (20, 4, "random"), (9, 8, "random"), (9, 8, "avoid"), (33, 2, "avoid"),
                                (5, 1, "random")]                                # appended, not reordered


def test_the_hand_laid_boards_below_16_cells_reach_their_leaves():
    """3x3 with two players: some row has a pending leaf below the root; 2x2 with one player: the root is pending and
    nothing below it is.  Both are consistent positions (every head on a cell of its own colour) with rows that differ."""
    for name, st, seat, agent, noise in CASES.tiny_states():
        assert st.N * st.N < 16 and st.B == 8 and len(set(st.tcount.tolist())) == 8
        assert len({(tuple(st.heads[:, b]), tuple(st.dirs[:, b])) for b in range(8)}) == 8
        for b in range(8):
            assert all(st.board[b, st.heads[p, b]] == p + 1 for p in range(st.P)) and len(set(st.heads[:, b].tolist())) == st.P
        count = R.new_count()
        root, seen = R.run(st, CASES.TINY_S, count=count, record=True, seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID, seat=seat,
                           agent=agent, noise=noise)
        assert (root["nodes"] > 0).all() and (root["sims"] == CASES.TINY_S).all() and seen[0]["pending"].all(), name
        below = sum(int(((s["pending"] == 1) & (s["depth"] > 0)).sum()) for s in seen)
        if st.P == 1:
            assert below == 0 and count["depth"] == 1 and count["terminal"] == 8 * (CASES.TINY_S - 1)
        else:
            assert below >= 1 and count["depth"] >= 2 and count["terminal"] > 0, (name, count)
            assert _replayed(st, seat, agent, noise, CASES.TINY_S) == below


def _waves(N):
    """the header's rule for `select`: one wave's LDS is the byte board rounded up to 16 bytes plus 16 bytes; a workgroup
    has as many waves as fit in 64 KB, four at the most"""
    wave_lds = (N * N + 15) // 16 * 16 + 16
    return min(4, 65536 // wave_lds), wave_lds


def test_the_lds_cases_stand_on_either_side_of_every_change_of_the_wave_count():
    waves = {N: _waves(N)[0] for N in range(2, 182)}                             # (181: the largest board a context takes)
    assert all(1 <= w <= 4 for w in waves.values())
    edges = sorted(N for N in range(2, 181) if waves[N] != waves[N + 1])
    assert edges == [127, 147, 180] and [waves[N] for N in (127, 128, 147, 148, 180, 181)] == [4, 3, 3, 2, 2, 1]
    assert sorted({N for N, P, B in CASES.LDS_CASES}) == sorted(edges + [N + 1 for N in edges])
    assert _waves(127) == (4, 16160) and 4 * 16160 == 64640 and _waves(181) == (1, 32784)
    for N, P, B in CASES.LDS_CASES:                                              # no wave count divides B: a ragged last workgroup
        assert waves[N] == 1 or B % waves[N], (N, B)
    assert (181, 8, 3) in CASES.LDS_CASES


@pytest.mark.parametrize("N, P, B", CASES.LDS_CASES, ids=CASES.LDS_IDS)
def test_the_lds_rows_search_open_mid_game_boards(N, P, B):
    st, seat = CASES.lds_state(N, P, B)
    count = R.new_count()
    root, seen = R.run(st, CASES.LDS_S, count=count, record=True, seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID, seat=seat,
                       agent="avoid", noise=CASES.NOISE)
    assert (root["nodes"] > 1).all() and (root["sims"] == CASES.LDS_S).all() and count["depth"] >= 3, count
    if N == 181:
        assert st.heads[0, 0] == N * N - 1 and st.heads[1, 1] > 32700 and st.heads[1, 1] // N == N - 1
        # the seat of row 0 leaves the board over the last cell (forward and right: terminal leaves), and pending leaves below
        # the root carry heads above 32,700 (row 1 along the last row)
        assert sum(1 for s in seen if not s["pending"][0]) >= 2
        assert any(s["pending"][1] and s["depth"][1] > 0 and s["leaf_heads"][1, 1] > 32700 for s in seen)
        assert any(s["pending"][b] and s["depth"][b] > 0 and s["obs_heads"][:, b].max() > 32700 for s in seen for b in range(B))


@pytest.mark.parametrize("row", CASES.CAPACITY, ids=[row["id"] for row in CASES.CAPACITY])
def test_the_capacity_rows_grow_large_trees(row):
    st = CASES.capacity_state()
    count = R.new_count()
    sr = R.Search(st, row["S"], seed=CASES.SEED, first_env_id=CASES.FIRST_ENV_ID, agent="avoid", noise=CASES.CAPACITY_NOISE, count=count)
    differ = 0
    for _ in range(row["S"]):
        leaves = sr.select(row["cpuct"])
        differ += not np.array_equal(leaves["obs_board"][0], leaves["obs_board"][1])
        sr.backup(*R.evaluator(leaves["obs_board"], leaves["obs_heads"], leaves["obs_dirs"]))
    print("\n%s: nodes %s, depth %d, greatest n below the root %s, greatest w %s, selects in which the rows differ %d"
          % (row["id"], [t.nodes for t in sr.trees], count["depth"], [max(t.n[1:]) for t in sr.trees], [max(t.w) for t in sr.trees], differ))
    assert max(t.nodes for t in sr.trees) >= row["reaches"]["nodes"]             # child indices above 255 (2048: above 11 bits)
    assert count["depth"] >= row["reaches"]["depth"]
    assert all(max(t.n[1:]) >= row["reaches"]["n"] for t in sr.trees)            # a node with n > 255
    assert max(max(t.w) for t in sr.trees) >= row["reaches"].get("w", 0)         # w sums within a factor of four of 4095 * 65536
    assert differ > row["S"] // 4                                                 # the two rows are two searches
    assert all(t.sims == row["S"] for t in sr.trees)
    sr.select(row["cpuct"])
    assert count["refused"] == 2


@pytest.mark.parametrize("agent", ["random", "avoid"])
def test_the_crash_rows_meet_every_kind_on_the_way_to_a_pending_leaf(agent):
    """every crash kind of tron_mcts_ref.CRASH_KINDS happens to a player other than the seat above a pending leaf, under each
    model; the same leaves are held to a replay with oracle.tron_step"""
    total = R.new_count()
    for N, P in CASES.CRASH_CASES:
        count = R.new_count()
        below = _replayed(CASES.state(N, P, CASES.CRASH_B), CASES.crash_seats(P, CASES.CRASH_B), agent, CASES.NOISE, CASES.CRASH_S,
                          count=count)
        assert below > CASES.CRASH_B
        for key in count:
            total[key] += count[key]
        if P == 8:                                                               # the eight-player rows meet the head-on kinds alone
            assert all(count["crash_" + kind] > 0 for kind in "def"), (N, P, count)
    print("\n%s: %s" % (agent, {kind: total["crash_" + kind] for kind in TM.CRASH_KINDS}))
    assert all(total["crash_" + kind] > 0 for kind in TM.CRASH_KINDS), total


def test_the_step_names_its_crash_kinds():
    """tron_mcts_ref.step's events on hand-laid 5x5 positions, one per kind, each also held to oracle.tron_step"""
    def play(P, heads, dirs, trail, dead, act):
        st = O.TronState(5, P, 1)
        for cell, v in trail.items():
            st.board[0, cell] = v
        for p, (h, d) in enumerate(zip(heads, dirs)):
            st.heads[p, 0], st.dirs[p, 0], st.board[0, h] = h, d, p + 1
        for p, k in dead.items():
            st.deaths[p, 0] = k
        pos, count = TM.pos_of(st, 0), {"events": []}
        TM.step(5, pos, act, count)
        O.tron_step(st, np.array(act, np.int8).reshape(P, 1))
        assert pos.board == st.board[0].tolist() and pos.h == st.heads[:, 0].tolist() and pos.k == st.deaths[:, 0].tolist()
        assert pos.d == [int(x) & 3 for x in st.dirs[:, 0]]
        return count["events"], pos
    # (a) off the board, (b) into another's trail, (c) into its own trail
    ev, pos = play(3, [0, 12, 24], [0, 1, 1], {13: 3, 19: 3, 23: 3}, {}, [0, 0, -1])
    assert ev == [("a", 0), ("b", 1), ("c", 2)] and pos.k == [1, 3, 3]
    # (d) + (g): player 0 runs into the live head of player 2, who then neither moves nor turns; (e): player 1 runs into the
    # head of player 3, dead before (killer id 4 overwritten with 2)
    ev, pos = play(4, [11, 21, 12, 22], [1, 1, 0, 0], {}, {3: 4}, [0, 0, 1, 0])
    assert ev == [("d", 2), ("e", 3), ("g", 2)] and pos.k == [3, 4, 1, 2] and pos.d == [1, 1, 0, 0]
    # (f): players 0 and 1 go for cell 12; the later one dies against the earlier one's new head, and kills it
    ev, pos = play(2, [11, 13], [1, 3], {}, {}, [0, 0])
    assert ev == [("d", 0), ("f", 1)] and pos.k == [2, 1] and pos.h == [12, 13] and pos.board[12] == 1
