"""Voronoi territory (crl_tron_territory) and the territory-greedy agent (crl_tron_sample_territory) on the host: every
CRL_EINVAL case of both C entries (rejected before any device work), the prototypes, the argument checks of the Python
wrappers, and the two numpy restatements of the header's contract (tests/territory_ref.py) against each other on seeded
mid-game positions and against hand-written answers."""
import ctypes as C

import numpy as np
import pytest

from tests import rng_ref
from tests import territory_ref as R
from tests.host_util import D, fake as _fake, lib as _lib, tron_context, ttt_context


def _terr(lib, ctx, B=4, state=(D,) * 4, seat=D, cand=D, A=1, outs=(D, D)):
    return lib.crl_tron_territory(ctx, B, *state, seat, cand, A, *outs, None)


def _agent(lib, ctx, B=4, tcount=D, noise=0.1, mask=3, state=(D,) * 4, actions=D):
    return lib.crl_tron_sample_territory(ctx, B, 1, 0, tcount, 1, noise, mask, *state, actions, None)


@pytest.fixture
def contexts():
    with tron_context() as h, ttt_context() as tt:
        yield _lib(), h, tt


def test_territory_argument_checks(contexts):
    lib, h, tt = contexts
    for i in range(4):                     # board, heads, dirs, deaths (seat may be NULL)
        st = [D] * 4
        st[i] = None
        assert _terr(lib, h, state=tuple(st)) == -1 and b"NULL" in lib.crl_last_error()
    for outs in ((None, D), (D, None)):
        assert _terr(lib, h, outs=outs) == -1 and b"NULL" in lib.crl_last_error()
    for B in (0, -1, (1 << 31) + 1):
        assert _terr(lib, h, B=B) == -1 and b"B=" in lib.crl_last_error()
    for A in (0, -1, 17, 65536):
        assert _terr(lib, h, A=A) == -1 and b"A=" in lib.crl_last_error()
    for A in (2, 3, 16):
        assert _terr(lib, h, cand=None, A=A) == -1 and b"cand" in lib.crl_last_error()
    assert _terr(lib, None) == -1 and b"tron context" in lib.crl_last_error()
    assert _terr(lib, tt) == -1 and b"tron context" in lib.crl_last_error()


def test_sample_territory_argument_checks(contexts):
    lib, h, tt = contexts
    assert _agent(lib, h, tcount=None) == -1 and b"NULL" in lib.crl_last_error()
    assert _agent(lib, h, actions=None) == -1 and b"NULL" in lib.crl_last_error()
    for i in range(4):
        st = [D] * 4
        st[i] = None
        assert _agent(lib, h, state=tuple(st)) == -1 and b"NULL" in lib.crl_last_error()
    for B in (0, -1, (1 << 31) + 1):
        assert _agent(lib, h, B=B) == -1 and b"B=" in lib.crl_last_error()
    for noise in (-0.01, 1.0001, float("nan"), float("inf")):
        assert _agent(lib, h, noise=noise) == -1 and b"noise" in lib.crl_last_error()
    for mask in (4, 7, 0x80000000):        # P = 2
        assert _agent(lib, h, mask=mask) == -1 and b"player_mask" in lib.crl_last_error()
    assert _agent(lib, None) == -1 and b"tron context" in lib.crl_last_error()
    assert _agent(lib, tt) == -1 and b"tron context" in lib.crl_last_error()


def test_prototypes_and_revision():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    assert len(_native.PROTOTYPES["crl_tron_territory"][1]) == 12
    assert _native.PROTOTYPES["crl_tron_sample_territory"] == _native.PROTOTYPES["crl_tron_sample_avoid"]


def test_territory_tag_words_match_the_oracle_philox():
    from oracle import oracle as O
    w = rng_ref.philox(np.array([7, 8]), np.array([3, 0xFFFFFFFF]), 2, R.TAG_TERRITORY, 0x1234567890ABCDEF)
    for i, (g, c) in enumerate(((7, 3), (8, 0xFFFFFFFF))):
        want = O.philox4x32([g, c, 2, rng_ref.CRL_TAG_TRON_TERRITORY], [0x90ABCDEF, 0x12345678])
        assert [int(x[i]) for x in w] == want.tolist()


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TronBatch
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    tb = _fake(TronBatch, B=5, P=3, N=7)
    ok = torch.zeros((5, 3), dtype=torch.int32)
    for cand in (torch.zeros((5, 3), dtype=torch.int64), torch.zeros((4, 3), dtype=torch.int32),
                 torch.zeros((5,), dtype=torch.int32), torch.zeros((5, 0), dtype=torch.int32),
                 torch.zeros((5, 17), dtype=torch.int32), np.zeros((5, 3), np.int32)):
        with pytest.raises(ValueError):
            tb.territory(cand)
    for seat in (torch.zeros((5,), dtype=torch.int32), torch.zeros((4,), dtype=torch.int8), np.zeros(5, np.int8), 0):
        with pytest.raises(ValueError):
            tb.territory(ok, seat)
        with pytest.raises(ValueError):
            tb.territory_action(seat)
    with pytest.raises(ValueError):        # an `out` dict with a wrong buffer, or without one
        tb.territory(ok, out={"area": torch.zeros((5, 3, 3), dtype=torch.int32), "info": torch.zeros((5, 3), dtype=torch.int32)})
    with pytest.raises(ValueError):
        tb.territory(ok, out={"area": torch.zeros((5, 3, 3), dtype=torch.int32)})
    for kw in ({"noise": -0.5}, {"noise": 1.5}, {"noise": float("nan")}, {"noise": "0.1"}, {"players": [3]}, {"players": [-1]},
               {"out": torch.zeros((3, 4), dtype=torch.int8)}, {"out": torch.zeros((3, 5), dtype=torch.int32)}):
        with pytest.raises(ValueError):
            tb.sample_territory(**kw)
    with pytest.raises(ValueError):        # (checked before the env builds its batch)
        TronSinglePlayerVectorEnv(15, 4, 8, opponent="greedy", device="cpu")


# ---- (i) == (ii) on seeded mid-game positions
@pytest.mark.parametrize("N", [4, 5, 13, 19, 20, 40])
def test_restatements_agree(N):
    for P in range(1, 9):
        for avoid in (False, True):
            B = 12
            st = R.positions(N, P, B, seed=100 * N + P, avoid=avoid)
            before = [x.copy() for x in (st.board, st.heads, st.dirs, st.deaths)]
            rng = np.random.default_rng(N + P)
            seat = rng.integers(-1, P + 1, size=B)
            cand = rng.integers(-1, 4, size=(B, 4))
            for kw in ({}, {"seat": seat, "cand": cand}, {"cand": np.tile(np.arange(3), (B, 1))}):
                a1, i1 = R.territory(N, st.board, st.heads, st.dirs, st.deaths, method="distance", **kw)
                a2, i2 = R.territory(N, st.board, st.heads, st.dirs, st.deaths, method="levels", **kw)
                assert np.array_equal(a1, a2) and np.array_equal(i1, i2), (N, P, avoid)
                # properties: areas are disjoint sets of free cells; dead players hold none; skipped rows are zeros
                free = (st.board == 0).sum(axis=1)
                assert (a2.sum(axis=2) <= free[:, None]).all()
                assert (a2[(st.deaths.T != 0)[:, None, :].repeat(a2.shape[1], axis=1)] == 0).all()
                assert (a2[i2 == 0] == 0).all()
                if "seat" in kw:
                    sk = (seat < 0) | (seat >= P)
                    sk |= st.deaths[np.clip(seat, 0, P - 1), np.arange(B)] != 0
                    skip = sk[:, None] | (cand < 0) | (cand > 2)
                    assert np.array_equal(i2 == 0, skip)
            assert all(np.array_equal(x, y) for x, y in zip(before, (st.board, st.heads, st.dirs, st.deaths)))   # read only


# ---- hand-written answers
def _areas(v, **kw):
    a1, i1 = R.territory(v["N"], v["board"], v["heads"], v["dirs"], v["deaths"], method="distance", **kw)
    a2, i2 = R.territory(v["N"], v["board"], v["heads"], v["dirs"], v["deaths"], method="levels", **kw)
    assert np.array_equal(a1, a2) and np.array_equal(i1, i2)
    return a2[0].tolist(), i2[0].tolist()


@pytest.mark.parametrize("N,P,each", [(15, 4, 48), (19, 4, 80), (20, 2, 189)])
def test_start_layout_is_shared_equally(N, P, each):
    from oracle import oracle as O
    sh, sd = O.tron_start_positions(N, P)
    st = O.TronState(N, P, 1)
    O.tron_reset(st, sh, sd)
    area, info = R.territory(N, st.board, st.heads, st.dirs, st.deaths)
    assert area.tolist() == [[[each] * P]] and info.tolist() == [[1]]
    # the cell behind every head is free there, and is no first cell
    free, first, _ = R.first_cells(N, st.board, st.heads, st.dirs, st.deaths)
    for p in range(P):
        x, y, d = int(sh[p]) % N, int(sh[p]) // N, (int(sd[p]) + 2) & 3
        bx, by = x + [0, 1, 0, -1][d], y + [-1, 0, 1, 0][d]
        assert free[0, by, bx] and not first[0, p, by, bx]
        assert first[0, p].sum() == 3


def test_hand_boards():
    hb = R.hand_boards()
    # ahead, right and left occupied: no first cell, although the cell behind and its row (3 cells) are free
    assert _areas(hb["behind"]) == ([[0]], [1])
    # walled in: 0; the other player reaches 18 of the 19 free cells (the corner behind the walls is cut off)
    assert _areas(hb["walled"]) == ([[0, 18]], [1])
    # the 19x19 spiral: 199 corridor cells, the head on the first, one new cell per level
    v = hb["spiral"]
    free, first, _ = R.first_cells(19, v["board"], v["heads"], v["dirs"], v["deaths"])
    area, depth = R.areas_by_levels(free, first)
    assert area.tolist() == [[198]] and depth.tolist() == [198] and depth[0] > 150
    assert _areas(v) == ([[198]], [1])
    # the corridor: two cells each; the middle cell and the two branch cells behind it belong to nobody (7 free cells)
    v = hb["corridor"]
    assert int((v["board"] == 0).sum()) == 7
    assert _areas(v) == ([[2, 2]], [1])
    # forced: forward as above; right / left of player 0 are walls: fatal (info 3), player 1 then takes all 7; padding skips
    got = _areas(v, seat=np.array([0]), cand=np.array([[0, 1, 2, -1, 3]]))
    assert got == ([[2, 2], [0, 7], [0, 7], [0, 0], [0, 0]], [1, 3, 3, 0, 0])
    # ... and the agent's rule on it: forward (score 0) beats the two fatal actions; player 1 likewise
    assert R.greedy_action(7, v["board"], v["heads"], v["dirs"], v["deaths"], np.array([0])).tolist() == [0]
    assert R.greedy_action(7, v["board"], v["heads"], v["dirs"], v["deaths"], np.array([1])).tolist() == [0]
    # a dead seat is skipped; a dead rival holds nothing and blocks nothing but its trail
    v["deaths"][1, 0] = 1
    assert _areas(v, seat=np.array([1]), cand=np.array([[0]])) == ([[0, 0]], [0])
    assert _areas(v) == ([[7, 0]], [1])


def test_agent_restatement_noise_extremes():
    st = R.positions(13, 3, 40, seed=5, avoid=True)
    g, c = np.arange(40) + 9, np.arange(40) * 3
    greedy = R.decide(13, st.board, st.heads, st.dirs, st.deaths, g, c, 77, 0.0)
    code = np.array([0, 1, -1], np.int8)
    for p in range(3):
        live = st.deaths[p] == 0
        want = code[R.greedy_action(13, st.board, st.heads, st.dirs, st.deaths, np.full(40, p))]
        assert np.array_equal(greedy[p][live], want[live]) and (greedy[p][~live] == 0).all()
    noisy = R.decide(13, st.board, st.heads, st.dirs, st.deaths, g, c, 77, 1.0)
    for p in range(3):
        w = rng_ref.philox(g, c, p, R.TAG_TERRITORY, 77)
        want = code[(w[1].astype(np.uint64) * np.uint64(3)) >> np.uint64(32)]
        assert np.array_equal(noisy[p], np.where(st.deaths[p] == 0, want, 0))
    only = R.decide(13, st.board, st.heads, st.dirs, st.deaths, g, c, 77, 0.0, players=[1])
    assert np.array_equal(only[1], greedy[1]) and (only[0] == 0).all() and (only[2] == 0).all()
