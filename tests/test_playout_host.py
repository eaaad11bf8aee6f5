"""Batched random playouts (crl_ttt_playout / crl_blokus_playout) on the host: the argument checks of the two C entry
points (every CRL_EINVAL case is rejected before any device work), the argument checks of the Python wrappers, and the
numpy restatement of the header's contract (tests/ttt_ref.py) against exact outcome probabilities of 3x3 positions
under uniform random play, computed here by recursion over the game tree."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import ttt_ref as R
from tests.host_util import D, fake as _fake, lib as _lib, ttt_context


def _ttt_call(lib, ctx, B=4, ptrs=None, cand=D, A=1, Rn=1, outs=None, flags=0):
    occ, winner, to_move, tcount = ptrs or (D, D, D, D)
    wins, played, len_sum = outs or (D, D, D)
    return lib.crl_ttt_playout(ctx, B, 1, 0, occ, winner, to_move, tcount, cand, A, Rn, wins, played, len_sum, flags, None)


def test_ttt_playout_argument_checks():
    lib = _lib()
    with ttt_context() as h:
        for i in range(3):                 # occ, winner, to_move (tcount may be NULL)
            ptrs = [D] * 4
            ptrs[i] = None
            assert _ttt_call(lib, h, ptrs=tuple(ptrs)) == -1 and b"NULL" in lib.crl_last_error()
        for i in range(3):
            outs = [D] * 3
            outs[i] = None
            assert _ttt_call(lib, h, outs=tuple(outs)) == -1 and b"NULL" in lib.crl_last_error()
        for B in (0, -1, (1 << 31) + 1):
            assert _ttt_call(lib, h, B=B) == -1 and b"B=" in lib.crl_last_error()
        for Rn in (0, -3, 65536):
            assert _ttt_call(lib, h, Rn=Rn) == -1 and b"R=" in lib.crl_last_error()
        for A in (0, -1, 65536):
            assert _ttt_call(lib, h, A=A) == -1 and b"A=" in lib.crl_last_error()
        assert _ttt_call(lib, h, cand=None, A=2) == -1 and b"cand" in lib.crl_last_error()
        for flags in (1, 8, 0x80000000):
            assert _ttt_call(lib, h, flags=flags) == -1 and b"flags" in lib.crl_last_error()
        assert _ttt_call(lib, None) == -1 and b"tictactoe" in lib.crl_last_error()
    with ttt_context(1, 1, 2, 2, 3) as small:  # fewer cells than players: refused as by crl_ttt_step_single
        assert _ttt_call(lib, small) == -1 and b"cells" in lib.crl_last_error()


def test_blokus_playout_argument_checks():
    lib = _lib()

    def call(state=(D,) * 6, cand=D, A=1, Rn=1, outs=(D,) * 4, flags=0, ctx=None, B=4):
        return lib.crl_blokus_playout(ctx, B, 1, 0, *state, cand, A, Rn, *outs, flags, None)
    with ttt_context() as tt:
        for i in range(5):                 # occ, inv, score, round, to_move (tcount may be NULL)
            st = [D] * 6
            st[i] = None
            assert call(state=tuple(st)) == -1 and b"NULL" in lib.crl_last_error()
        for i in range(4):
            outs = [D] * 4
            outs[i] = None
            assert call(outs=tuple(outs)) == -1 and b"NULL" in lib.crl_last_error()
        for Rn in (0, 65536):
            assert call(Rn=Rn) == -1 and b"R=" in lib.crl_last_error()
        for A in (0, 65536):
            assert call(A=A) == -1 and b"A=" in lib.crl_last_error()
        assert call(cand=None, A=3) == -1 and b"cand" in lib.crl_last_error()
        for flags in (1, 2, 0x80000000):
            assert call(flags=flags) == -1 and b"flags" in lib.crl_last_error()
        # every argument right but the context: none, or one of another game
        assert call() == -1 and b"blokus context" in lib.crl_last_error()
        assert call(ctx=tt) == -1 and b"blokus context" in lib.crl_last_error()


def test_playout_prototypes():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113
    assert "crl_ttt_playout" in _native.PROTOTYPES and "crl_blokus_playout" in _native.PROTOTYPES


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def test_ttt_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TTTBatch
    tb = _fake(TTTBatch, B=5, P=2, n_cells=9)
    ok = torch.zeros((5, 9), dtype=torch.int32)
    for bad in (0, 65536, -1, 2.0, True):
        with pytest.raises(ValueError):
            tb.playout(bad)
    for cand in (torch.zeros((5, 9), dtype=torch.int64), torch.zeros((4, 9), dtype=torch.int32),
                 torch.zeros((5,), dtype=torch.int32), torch.zeros((5, 0), dtype=torch.int32), ok.t().contiguous().t(),
                 np.zeros((5, 9), np.int32)):
        with pytest.raises(ValueError):
            tb.playout(3, cand)
    with pytest.raises(ValueError):        # an `out` dict with a wrong buffer
        tb.playout(3, ok, out={"wins": torch.zeros((5, 9, 3), dtype=torch.int32), "draws": torch.zeros((5, 9), dtype=torch.int32),
                               "played": torch.zeros((5, 9), dtype=torch.int32), "len_sum": torch.zeros((5, 9), dtype=torch.int32)})
    with pytest.raises(ValueError):
        tb.playout(3, ok, out={"wins": torch.zeros((5, 9, 2), dtype=torch.int32)})
    with pytest.raises(ValueError):
        tb.flat_mc_action(0)


def test_blokus_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    bb = _fake(BlokusBatch, B=3, P=4)
    ok = torch.zeros((3, 4), dtype=torch.int32)
    for bad in (0, 70000):
        with pytest.raises(ValueError):
            bb.playout(bad)
    for cand in (torch.zeros((3, 4), dtype=torch.int16), torch.zeros((2, 4), dtype=torch.int32)):
        with pytest.raises(ValueError):
            bb.playout(2, cand)
        with pytest.raises(ValueError):
            bb.flat_mc_action(cand, 2)
    with pytest.raises(ValueError):        # score_sum is part of the Blokus dict
        bb.playout(2, ok, out={k: torch.zeros(s, dtype=torch.int32) for k, s in
                               (("wins", (3, 4, 4)), ("draws", (3, 4)), ("played", (3, 4)), ("len_sum", (3, 4)))})
    with pytest.raises(ValueError):
        bb.flat_mc_action(ok, 65536)


# ---- the restatement against exact outcome probabilities
POSITIONS = [(0, 0, 0),                                   # the empty board
             (0b000010000, 0, 1),                         # X in the centre, O to move
             (0b000000011, 0b000011000, 0),               # X can complete the top row
             (0b100000001, 0b000010000, 1),               # X in two corners, O in the centre
             (0b010001100, 0b001100010, 0)]               # late, two empty cells


def _ttt_state(positions):
    from oracle import oracle as O
    st = O.TTTState((3, 3), 3, 2, len(positions))
    for b, (x, o, m) in enumerate(positions):
        st.occ[0, b], st.occ[1, b], st.to_move[b] = x, o, m
    return st


def test_restatement_matches_exact_probabilities():
    Rn, seed = 1500, 0xC0FFEE
    st = _ttt_state(POSITIONS)
    before = (st.occ.copy(), st.winner.copy(), st.to_move.copy())
    wins, played, len_sum = R.playout(st, seed, Rn, R.random_agent, first_env_id=11, tcount=np.array([0, 5, 9, 2, 7], np.uint32))
    assert np.array_equal(st.occ, before[0]) and np.array_equal(st.to_move, before[2])   # inputs are read only
    assert (played[:, 0] == Rn).all()
    for b, (x, o, m) in enumerate(POSITIONS):
        p = R.exact_3x3(x, o, m)
        for q, pq in enumerate(p + (1.0 - sum(p),)):
            n = int(wins[b, 0, q]) if q < 2 else Rn - int(wins[b, 0].sum())
            sigma = math.sqrt(Rn * pq * (1 - pq))
            assert abs(n - Rn * pq) <= 6 * sigma + 1, (b, q, n, Rn * pq)
        empties = 9 - bin(x | o).count("1")
        assert Rn <= len_sum[b, 0] <= Rn * empties


def test_restatement_candidates_and_skips():
    from oracle import oracle as O
    st = _ttt_state([(0b000000011, 0b000011000, 0), (0b000000111, 0b000011000, 1)])   # b = 1: X has won
    st.winner[1] = 0
    cand = np.array([[2, 0, -1, 9, 8], [5, 6, 7, 8, -1]], np.int64)
    wins, played, len_sum = R.playout(st, 3, 40, R.random_agent, cand=cand, A=5)
    assert list(played[0]) == [40, 0, 0, 0, 40] and (played[1] == 0).all()
    assert wins[0, 0, 0] == 40 and len_sum[0, 0] == 40          # cell 2 completes X's row: one ply, always won
    assert (wins[1] == 0).all() and (len_sum[1] == 0).all()
    # the candidate ply is a move of the mover, the random plies follow it
    one = R.one_game(st, 0)
    O.ttt_step(one, np.array([8], np.int8))
    p = R.exact_3x3(int(one.occ[0, 0]), int(one.occ[1, 0]), 1)
    sigma = math.sqrt(40 * p[0] * (1 - p[0]))
    assert abs(int(wins[0, 4, 0]) - 40 * p[0]) <= 6 * sigma + 1
