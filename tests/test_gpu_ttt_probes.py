"""One-ply probes of the TicTacToe win test on the GPU (tests/ttt_probes.py): every non-zero mask of the boards of at most
16 cells, and every line, near-line, wrap run, the top bit and 50,000 random masks of the larger ones, completed by one
ply through every entry point that tests for a line -- crl_ttt_step, crl_ttt_step_observe, crl_ttt_step_board,
crl_ttt_step_single and crl_ttt_playout, the last two with the win-mask table and without.  One launch per call; the
verdicts are the numpy predicate's, the full outputs the oracle's (tests/test_ttt_probes_host.py holds the two together).
Then the row shapes of the playout kernel -- rows inside a wave, rows that are whole waves, rows across waves and
workgroups -- against the numpy restatement."""
import numpy as np
import pytest
import torch

from tests import ttt_ref
from tests import ttt_probes as TP
from tests.gpu_util import DEV, np_of as _np, to_dev as _dev, ttt_batch, u32_of as _u32

pytestmark = pytest.mark.gpu

SMALL = [(d, k, p, dens) for d, k, p, dens in TP.PROBE_SHAPES if TP.n_cells_of(d) <= 16]
SMALL_IDS = [TP.shape_id(d, k, p) for d, k, p, _ in SMALL]


def _batch(dims, K, P, pr):
    """a TTTBatch in the probe state"""
    from colosseumrl_amd.batched import TTTBatch
    tb = TTTBatch(dims, K, P, len(pr["masks"]), device=DEV)
    tb.occ.copy_(_dev(pr["occ"]))
    tb.to_move.copy_(_dev(pr["to_move"]))
    return tb


def _same_state(tb, orc):
    assert np.array_equal(_u32(tb.occ), orc["occ"])
    assert np.array_equal(_np(tb.winner), orc["winner"]) and np.array_equal(_np(tb.to_move), orc["to_move"])


def _same_step(reward, terminal, winners, orc):
    assert np.array_equal(_np(reward), orc["reward"]) and np.array_equal(_np(terminal), orc["terminal"])
    assert np.array_equal(_np(winners), orc["winners"])


def _relative(board, rel, P):
    bd = board.astype(np.int16)
    return np.where(bd >= 0, (bd - rel.astype(np.int16)[:, None]) % P, -1).astype(np.int8)


# ------------------------------------------------------------------ the step entry points
@pytest.mark.parametrize("dims,K,P,density", TP.PROBE_SHAPES, ids=TP.PROBE_IDS)
def test_step_entry_points(dims, K, P, density):
    from colosseumrl_amd.batched import TTTBoards
    pr, orc = TP.probes_of(dims, K, P, density), TP.oracle_step_of(dims, K, P, density)
    action = _dev(pr["action"])
    assert np.array_equal(orc["winner"] == pr["to_move"], pr["want"])         # the verdicts compared below are the predicate's

    tb = _batch(dims, K, P, pr)                                               # crl_ttt_step, then crl_ttt_valid / _board
    _same_step(*tb.step(action), orc)
    _same_state(tb, orc)
    assert np.array_equal(_u32(tb.valid_mask()), orc["valid"]) and np.array_equal(_np(tb.board()), orc["board"])

    tb = _batch(dims, K, P, pr)                                               # crl_ttt_step_observe, external actions
    out = tb.step_observe(action, auto_reset=False)
    _same_step(out["reward"], out["terminal"], out["winners"], orc)
    _same_state(tb, orc)
    assert np.array_equal(_u32(out["valid"]), orc["valid"])
    assert np.array_equal(_np(out["board"]), _relative(orc["board"], orc["to_move"], P))

    bb = TTTBoards(dims, K, P, len(pr["masks"]), device=DEV)                  # crl_ttt_step_board: the reference's layout
    bb.board.copy_(_dev(orc["board_before"]))
    bb.to_move.copy_(_dev(pr["to_move"]))
    _same_step(*bb.step(action), orc)
    assert np.array_equal(_np(bb.board), orc["board"]) and np.array_equal(_np(bb.winner), orc["winner"])
    assert np.array_equal(_np(bb.to_move), orc["to_move"]) and np.array_equal(_u32(bb.valid), orc["valid"])
    assert np.array_equal(_np(bb.obs), _relative(orc["board"], orc["to_move"], P))


# ------------------------------------------------------------------ step_single and playout
def _single_and_playout(dims, K, P, density):
    pr = TP.probes_of(dims, K, P, density)
    want, mover, B = pr["want"], pr["to_move"], len(pr["masks"])
    # the learner sits where the mover is and plays the probe's cell: one learner ply per call, and no later ply of the
    # call can win for the learner, so the reward is +1 exactly where that ply completes a line
    tb = _batch(dims, K, P, pr)
    out = tb.step_single(_dev(mover), _dev(pr["action"].astype(np.int64)), seed=5)
    reward = _np(out["reward"])
    assert np.array_equal(reward == 1, want)
    assert _np(out["done"])[want | pr["full"]].all()
    assert np.array_equal(_np(out["winners"])[want], mover[want])
    # a playout row whose candidate is the probe's cell: one ply long exactly where that ply ends the game
    tb = _batch(dims, K, P, pr)
    before = [t.clone() for t in (tb.occ, tb.winner, tb.to_move, tb.tcount)]
    po = tb.playout(1, _dev(pr["action"].astype(np.int32).reshape(B, 1)), seed=7)
    wins, played, len_sum = _u32(po["wins"]), _u32(po["played"]), _u32(po["len_sum"])
    assert (played == 1).all()
    assert np.array_equal((wins[np.arange(B), 0, mover] == 1) & (len_sum[:, 0] == 1), want)
    assert np.array_equal(len_sum[:, 0] == 1, want | pr["full"])
    assert (wins.sum(axis=2) <= 1).all() and (wins.sum(axis=(1, 2))[pr["full"] & ~want] == 0).all()
    for a, b in zip(before, (tb.occ, tb.winner, tb.to_move, tb.tcount)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dims,K,P,density", TP.PROBE_SHAPES, ids=TP.PROBE_IDS)
def test_step_single_and_playout(dims, K, P, density):
    _single_and_playout(dims, K, P, density)


@pytest.mark.parametrize("dims,K,P,density", SMALL, ids=SMALL_IDS)
def test_step_single_and_playout_without_the_win_table(dims, K, P, density, monkeypatch):
    """boards of at most 16 cells on contexts made without the table of winning masks: the shift-and test"""
    monkeypatch.setenv("CRL_TTT_NO_WIN_TABLE", "1")
    _single_and_playout(dims, K, P, density)


# ------------------------------------------------------------------ playout row shapes
@pytest.mark.parametrize("Rn,A", [(2, 3), (32, 2), (63, 1), (64, 2), (128, 1), (130, 1)])
def test_playout_row_shapes(Rn, A):
    """Rows of R lanes: several per wave (R = 2, 32), one lane short of a wave (63), whole waves (64), two waves (128),
    two waves and two lanes (130).  B is the smallest with a lane in a second 256-lane workgroup, so that rows lie inside
    a wave, across waves and -- where R does not divide 256 -- across workgroups; positions that are over and candidates
    that are not empty cells leave skipped rows among the played ones."""
    dims, K, P = (3, 3), 3, 2
    B = 256 // (Rn * A) + 1
    assert B * A * Rn > 256 and (B - 1) * A * Rn <= 256
    rng = np.random.default_rng(Rn * 10 + A)
    seed, first_env_id = 77 + Rn, 300
    st = TP.random_positions(dims, K, P, B, rng)
    for b in range(min(B, 2)):                                               # the first rows are played whatever the draw
        st.occ[:, b], st.winner[b], st.to_move[b] = 0, -1, b % P
    tcount = rng.integers(0, 1000, size=B).astype(np.uint32)
    cand = rng.integers(-1, 10, size=(B, A))
    cand[0, 0] = 4
    tb = ttt_batch(st, first_env_id, tcount)
    out = tb.playout(Rn, _dev(cand.astype(np.int32)), seed)
    wins, played, len_sum = ttt_ref.playout(st, seed, Rn, ttt_ref.random_agent, cand=cand, A=A, first_env_id=first_env_id, tcount=tcount)
    assert played.any()
    assert np.array_equal(_u32(out["played"]), played) and np.array_equal(_u32(out["wins"]), wins)
    assert np.array_equal(_u32(out["len_sum"]), len_sum)
    if A == 1:                                                               # and without candidates
        out = tb.playout(Rn, None, seed)
        wins, played, len_sum = ttt_ref.playout(st, seed, Rn, ttt_ref.random_agent, first_env_id=first_env_id, tcount=tcount)
        assert np.array_equal(_u32(out["played"]), played) and np.array_equal(_u32(out["wins"]), wins)
        assert np.array_equal(_u32(out["len_sum"]), len_sum)
