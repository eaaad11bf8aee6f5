"""The one-ply probes of the TicTacToe win test (tests/ttt_probes.py) on the host: the numpy predicate against every record
the reference left in the fixtures, the oracle's ply against the predicate on every probe shape, the conditions that keep
the GPU probe tests from passing vacuously, and the numpy restatements of step_single and playout run alone on every row
of the instance table, at the sizes of the GPU tests, for the episode conditions those tests rely on."""
import numpy as np
import pytest

from tests import ttt_ref
from tests import ttt_probes as TP

TRAJ = ["ttt_traj_%dp_%s" % (p, r) for p in (2, 3, 4) for r in ("reset", "noreset")]


# ------------------------------------------------------------------ the predicate against the reference
def _check_records(dims, K, P, board, winner):
    board, winner = board.reshape(-1, board.shape[-1]), winner.reshape(-1)
    assert board.shape[1] == TP.n_cells_of(dims) and len(board) == len(winner)
    for p in range(P):
        got = TP.has_line(dims, K, TP.pack(board == p))
        assert np.array_equal(got, winner == p), p             # a line exactly when p is the record's winner
    return int((winner >= 0).sum()), int((winner < 0).sum())


@pytest.mark.parametrize("name", TRAJ)
def test_predicate_on_trajectory_fixtures(golden, name):
    g = golden(name)
    dims = tuple(int(x) for x in g["shape"])
    won, running = _check_records(dims, int(g["K"]), int(g["P"]), g["board"], g["winner"])
    assert won > 0 and running > 0


@pytest.mark.parametrize("which,dims,P", [("ttt2", (3, 3), 2), ("ttt3", (3, 5), 3), ("ttt4", (3, 3, 3), 4)])
def test_predicate_on_live_fixtures(golden, which, dims, P):
    g = golden("live_" + which)
    assert tuple(g["dims"]) == dims
    won, running = _check_records(dims, 3, P, g["board"], g["winner"])
    assert won > 0 and running > 0


def test_predicate_small_cases():
    assert TP.has_line((3, 3), 3, [0b111, 0b001010100, 0b100010001, 0b001001001]).all()
    assert not TP.has_line((3, 3), 3, [0b011, 0b000001110, 0b110001000, 0b101101010]).any()
    assert not TP.has_line((3, 5), 3, [0b1110000]).any()                     # cells 4, 5, 6: off the end of a row
    assert TP.wrap_runs((3, 5), 3).count(0b1110000) == 1
    assert TP.has_line((3, 3, 3), 3, [1 | 1 << 13 | 1 << 26, 1 << 2 | 1 << 13 | 1 << 24]).all()   # space diagonals
    assert len(TP.directions()) == 13 and TP.n_directions((3, 3, 3), 3) == 13 and TP.n_directions((2, 4, 4), 3) == 4
    assert [len(TP.line_masks(d, k)) for d, k in (((3, 3), 3), ((3, 5), 3), ((3, 3, 3), 3), ((5, 5), 4))] == [8, 20, 49, 28]


# ------------------------------------------------------------------ the oracle against the predicate
@pytest.mark.parametrize("dims,K,P,density", TP.PROBE_SHAPES, ids=TP.PROBE_IDS)
def test_oracle_ply_against_predicate(dims, K, P, density):
    from oracle import oracle as O
    pr, orc = TP.probes_of(dims, K, P, density), TP.oracle_step_of(dims, K, P, density)
    assert sorted(int(x) for x in O.ttt_lines(*TP.dims3(dims), K)) == TP.line_masks(dims, K)
    want, mover, full = pr["want"], pr["to_move"], pr["full"]
    assert np.array_equal(orc["winner"], np.where(want, mover, -1))          # winner == mover exactly where want
    assert np.array_equal(orc["reward"], want.astype(np.int8))               # the header's rule: +1 for the mover's win,
    assert np.array_equal(orc["winners"], np.where(want, mover, -1))         # the winner named, terminal on a win or a
    assert np.array_equal(orc["terminal"].astype(bool), want | full)         # full board
    assert np.array_equal(orc["terminal"].astype(bool) & (orc["winners"] < 0), full & ~want)
    assert np.array_equal(orc["to_move"], (mover.astype(np.int64) + 1) % P)
    after = pr["occ"].copy()
    after[mover, np.arange(len(mover))] = pr["masks"]
    assert np.array_equal(orc["occ"], after)


# ------------------------------------------------------------------ conditions on the probe sets
@pytest.mark.parametrize("dims,K,P,density", TP.PROBE_SHAPES, ids=TP.PROBE_IDS)
def test_probe_set_conditions(dims, K, P, density):
    """Each verdict at least 300 times on a shape that has a line; the movers, the played cells and the fillings spread;
    wrap runs rejected unless the mask holds a line besides; bit 31 in both verdicts.  A 2-D board has few wrap runs (8 on
    3x9 K 3, 24 on 5x5 K 4, 120 on 3x3x3 K 3): each is probed bare and under random extra cells of the same player, so
    that at least 100 masks per shape hold one."""
    pr = TP.probes_of(dims, K, P, density)
    n, masks, want = TP.n_cells_of(dims), pr["masks"], pr["want"]
    lines = np.array(TP.line_masks(dims, K), np.uint32)
    if len(lines):
        assert int(want.sum()) >= 300 and int((~want).sum()) >= 300, (int(want.sum()), int((~want).sum()))
    else:
        assert not want.any()
    assert (masks != 0).all() and (masks <= TP.full_mask(dims)).all()
    if n <= 16:
        assert set(int(m) for m in masks) == set(range(1, 1 << n))           # every non-zero mask
    else:
        have = set(int(m) for m in masks)
        assert have.issuperset(int(x) for x in lines) and int((~pr["is_wrap"]).sum()) >= TP.RANDOM_MASKS
    # the probes themselves: one bit of the mask played, the masks disjoint, the cell empty, every mover, both fillings
    bit = np.uint32(1) << pr["action"].astype(np.uint32)
    mine = pr["occ"][pr["to_move"], np.arange(len(masks))]
    assert np.array_equal(mine | bit, masks) and not (mine & bit).any()
    assert int(pr["occ"].astype(np.uint64).sum(axis=0).max()) <= TP.full_mask(dims)
    assert np.array_equal(np.bitwise_or.reduce(pr["occ"], axis=0).astype(np.uint64), pr["occ"].astype(np.uint64).sum(axis=0))
    assert set(pr["to_move"].tolist()) == set(range(P))
    assert len(set(pr["action"].tolist())) == n
    lowest = (masks & (~masks + np.uint32(1))) == bit
    assert 0 < int((~lowest).sum())                                          # not always the lowest bit
    assert pr["full"].any() and (~pr["full"]).any()
    if P > 1:
        others = np.bitwise_or.reduce(pr["occ"], axis=0) & ~mine
        assert (others == 0).any() and pr["full"].sum() >= 300
    # wrap runs
    runs = TP.wrap_runs(dims, K)
    wrap = pr["is_wrap"]
    if n > 16 and sum(d > 1 for d in TP.dims3(dims)) >= 2:
        assert len(runs) >= 8 and int(wrap.sum()) >= TP.MIN_WRAP_RUNS
        assert have.issuperset(runs)
    if wrap.any():
        run_of = np.array(runs * (int(wrap.sum()) // len(runs)), np.uint32)
        assert np.array_equal(masks[wrap] & run_of, run_of)                  # each of these masks holds its run
        other_line = ((masks[wrap][:, None] & lines[None, :]) == lines[None, :]).any(axis=1)
        assert np.array_equal(want[wrap], other_line)                        # a win only by a line that is there besides
        assert not want[wrap][:len(runs)].any() and int((~want[wrap]).sum()) >= len(runs)
    if n == 32:
        top = (masks >> np.uint32(31)).astype(bool)
        assert (top & want).any() and (top & ~want).any()
        assert ((pr["action"] == 31) & want).any() and ((pr["action"] == 31) & ~want).any()


def test_probe_shape_table_covers_the_paths():
    rows = [(d, k, p) for d, k, p, _ in TP.PROBE_SHAPES]
    ks = {k for _, k, _ in rows}
    assert {2, 3, 4, 5, 6} <= ks and any(k >= 7 for k in ks)
    fam = {TP.family_of(d, k) for d, k, _ in rows}
    assert fam == {"table", "nd4", "nd13"}
    assert {sum(x > 1 for x in TP.dims3(d)) for d, _, _ in rows} >= {1, 2, 3}
    assert sum(TP.n_cells_of(d) == 32 for d, _, _ in rows) >= 3
    assert any(len(TP.line_masks(d, k)) == 1 for d, k, _ in rows) and any(len(TP.line_masks(d, k)) == 0 for d, k, _ in rows)
    for fam_k in (("nd4", 3), ("nd4", 4), ("nd4", 5), ("nd4", 6), ("nd13", 2), ("nd13", 3), ("table", 5)):
        assert any((TP.family_of(d, k), k) == fam_k for d, k, _ in rows), fam_k


def test_instance_table_covers_every_instance():
    assert len(TP.INSTANCE_ROWS) == 24 and len(set(TP.INSTANCE_IDS)) == 24
    seen = {(TP.family_of(d, k), p) for d, k, p in TP.INSTANCE_ROWS}
    assert seen == {(f, p) for f in ("table", "nd4", "nd13") for p in range(1, 9)}
    assert all(TP.n_cells_of(d) >= p for d, _, p in TP.INSTANCE_ROWS)
    ks = {k for _, k, _ in TP.INSTANCE_ROWS}
    assert {3, 4, 5} <= ks and ks - {3, 4, 5}
    for old in ("3x3k3p2", "3x5k3p3", "3x3x3k3p4", "5x5k4p3"):                # the rows the suite ran before the table
        assert old in TP.INSTANCE_IDS
    assert [r for r, _, _, _ in TP.PLAYOUT_CASES] == TP.INSTANCE_ROWS


# ------------------------------------------------------------------ the restatements alone, at the GPU tests' sizes
def _valid_by_hand(st):
    out = []
    for b in range(st.B):
        taken = 0
        for p in range(st.P):
            taken |= int(st.occ[p, b])
        out.append(((1 << st.n_cells) - 1) & ~taken)
    return out


@pytest.mark.parametrize("mixed", [False, True], ids=["fixed_seat", "mixed_seats"])
@pytest.mark.parametrize("dims,K,P", TP.INSTANCE_ROWS, ids=TP.INSTANCE_IDS)
def test_step_single_restatement_on_the_instance_table(dims, K, P, mixed):
    """What tests/test_gpu_single_turn.py::test_ttt_against_restatement does on the host side: some game ends within its
    18 calls, and on 32 cells the valid masks keep all 32 bits."""
    from oracle import oracle as O
    B, seed = 37, 1234 + P
    st = O.TTTState(dims, K, P, B)
    rng = np.random.default_rng(P * 10 + mixed)
    seat = (rng.integers(0, P, size=B) if mixed else np.full(B, P - 1)).astype(np.int8)
    ttt_ref.step_single(st, seat, None, seed, ttt_ref.random_agent)
    n_done = 0
    for _ in range(18):
        act = TP.single_turn_actions(st, rng)
        reward, done, winners, obs, valid = ttt_ref.step_single(st, seat, act, seed, ttt_ref.random_agent)
        n_done += int(done.sum())
        assert valid.dtype == np.uint32 and valid.tolist() == _valid_by_hand(st)
        assert all(int(st.to_move[b]) == seat[b] for b in range(B))
        assert ((obs >= -1) & (obs < P)).all() and np.array_equal(obs < 0, st.board() < 0)
    assert n_done > 0


@pytest.mark.parametrize("cfg,r_cand,r_none,n_cand", TP.PLAYOUT_CASES, ids=TP.INSTANCE_IDS)
def test_playout_restatement_on_the_instance_table(cfg, r_cand, r_none, n_cand):
    """What tests/test_gpu_playout.py::test_ttt_against_restatement computes on the host side: played and skipped rows
    with and without candidates, and on 32 cells playouts that reach cell 31."""
    st, tcount, rng, first_env_id, seed = TP.playout_case_inputs(cfg)
    n = st.n_cells
    cand = TP.playout_candidates(n, st.B, rng, n_cand)
    assert cand.shape[1] == (n if n_cand is None else n_cand) + 4
    wins, played, len_sum = ttt_ref.playout(st, seed, r_cand, ttt_ref.random_agent, cand=cand, A=cand.shape[1], first_env_id=first_env_id,
                                                    tcount=tcount)
    assert played.any() and not played.all() and set(np.unique(played)) == {0, r_cand}
    empty = np.array(_valid_by_hand(st), np.uint64)
    ok = (cand >= 0) & (cand < n) & (((empty[:, None] >> np.clip(cand, 0, 31).astype(np.uint64)) & 1) == 1)
    running = (st.winner < 0) & (empty != 0)
    assert np.array_equal(played > 0, ok & running[:, None])                 # a row is played exactly on an empty cell of a
    assert (wins.sum(axis=2) <= played).all() and (len_sum >= played).all()  # running game
    if n == 32:
        assert (played[cand == 31] > 0).any()
    wins, played, len_sum = ttt_ref.playout(st, seed, r_none, ttt_ref.random_agent, first_env_id=first_env_id, tcount=tcount)
    assert played.any() and not played.all()
    assert np.array_equal(played[:, 0] > 0, running)
    assert (len_sum[played > 0] <= r_none * np.array([bin(int(e)).count("1") for e in empty])[played[:, 0] > 0]).all()
