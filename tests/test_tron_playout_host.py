"""Batched Tron playouts (crl_tron_playout) on the host: every CRL_EINVAL case of the C entry (rejected before any device
work), the argument checks of the Python wrappers, the prototype, and the numpy restatement of the header's contract
(tests/tron_ref.py) against exact outcome probabilities of tiny boards under uniform random play, computed here
by memoised recursion over the 3^alive joint actions."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import tron_ref as TR
from tests.host_util import D, fake as _fake, lib as _lib, tron_context, ttt_context


def _call(lib, ctx, B=4, state=(D,) * 4, tcount=D, seat=D, cand=D, A=1, Rn=1, noise=0.1, max_steps=0, outs=(D,) * 4,
          flags=0):
    return lib.crl_tron_playout(ctx, B, 1, 0, *state, tcount, seat, cand, A, Rn, noise, max_steps, *outs, flags, None)


def test_tron_playout_argument_checks():
    lib = _lib()
    with tron_context() as h, ttt_context() as tt:
        for i in range(4):                 # board, heads, dirs, deaths (tcount and seat may be NULL)
            st = [D] * 4
            st[i] = None
            assert _call(lib, h, state=tuple(st)) == -1 and b"NULL" in lib.crl_last_error()
        for i in range(4):
            outs = [D] * 4
            outs[i] = None
            assert _call(lib, h, outs=tuple(outs)) == -1 and b"NULL" in lib.crl_last_error()
        for B in (0, -1, (1 << 31) + 1):
            assert _call(lib, h, B=B) == -1 and b"B=" in lib.crl_last_error()
        for Rn in (0, -3, 65536):
            assert _call(lib, h, Rn=Rn) == -1 and b"R=" in lib.crl_last_error()
        for A in (0, -1, 65536):
            assert _call(lib, h, A=A) == -1 and b"A=" in lib.crl_last_error()
        assert _call(lib, h, cand=None, A=3) == -1 and b"cand" in lib.crl_last_error()
        for noise in (-0.01, 1.0001, float("nan"), float("inf")):
            assert _call(lib, h, noise=noise) == -1 and b"noise" in lib.crl_last_error()
        for ms in (-1, 65536):
            assert _call(lib, h, max_steps=ms) == -1 and b"max_steps" in lib.crl_last_error()
        for flags in (4, 8, 0x80000000, 7):
            assert _call(lib, h, flags=flags) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, None) == -1 and b"tron context" in lib.crl_last_error()
        assert _call(lib, tt) == -1 and b"tron context" in lib.crl_last_error()


def test_tron_playout_prototype():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113
    assert "crl_tron_playout" in _native.PROTOTYPES
    assert (_native.CRL_PLAYOUT_AVOID, _native.CRL_PLAYOUT_UNTIL_SEAT_DONE) == (1, 2)


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def test_tron_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TronBatch
    tb = _fake(TronBatch, B=5, P=3, N=7)
    ok = torch.zeros((5, 3), dtype=torch.int32)
    for bad in (0, 65536, -1, 2.0, True):
        with pytest.raises(ValueError):
            tb.playout(bad)
        with pytest.raises(ValueError):
            tb.flat_mc_action(bad)
    for cand in (torch.zeros((5, 3), dtype=torch.int64), torch.zeros((4, 3), dtype=torch.int32),
                 torch.zeros((5,), dtype=torch.int32), torch.zeros((5, 0), dtype=torch.int32), np.zeros((5, 3), np.int32)):
        with pytest.raises(ValueError):
            tb.playout(3, cand)
    for kw in ({"agent": "greedy"}, {"until": "never"}, {"noise": -0.5}, {"noise": 1.5}, {"noise": float("nan")},
               {"noise": "0.1"}, {"max_steps": -1}, {"max_steps": 65536}, {"max_steps": 2.0},
               {"seat": torch.zeros((5,), dtype=torch.int32)}, {"seat": torch.zeros((4,), dtype=torch.int8)},
               {"seat": np.zeros(5, np.int8)}):
        with pytest.raises(ValueError):
            tb.playout(3, ok, **kw)
    with pytest.raises(ValueError):        # an `out` dict with a wrong buffer, or without one
        tb.playout(3, ok, out={"wins": torch.zeros((5, 3, 2), dtype=torch.int32), "played": torch.zeros((5, 3), dtype=torch.int32),
                               "len_sum": torch.zeros((5, 3), dtype=torch.int32), "ret_sum": torch.zeros((5, 3), dtype=torch.int32)})
    with pytest.raises(ValueError):
        tb.playout(3, ok, out={"wins": torch.zeros((5, 3, 3), dtype=torch.int32)})


# ---- the restatement against exact outcome probabilities (random agent, play to the end)
def _py_step(N, P, board, h, d, k, act):
    """CyTronGrid.pyx:15-62 + TronGridEnvironment.py:309-321 on tuples -> (board, h, d, k, terminal, winners mask)"""
    board, h, d, k = [int(v) for v in board], [int(v) for v in h], [int(v) for v in d], [int(v) for v in k]
    for i in range(P):
        if k[i] > 0:
            continue
        x, y = h[i] % N, h[i] // N
        dr = (d[i] + act[i] + 4) % 4
        x += (dr == 1) - (dr == 3)
        y += (dr == 2) - (dr == 0)
        d[i] = dr
        if not (0 <= x < N and 0 <= y < N):
            k[i] = i + 1
        elif board[y * N + x] > 0:
            e = board[y * N + x]
            k[i] = e
            if h[e - 1] == y * N + x:
                k[e - 1] = i + 1
        else:
            board[y * N + x] = i + 1
            h[i] = y * N + x
    alive = [i for i in range(P) if k[i] == 0]
    term = len(alive) <= 1
    return tuple(board), tuple(h), tuple(d), tuple(k), term, (sum(1 << i for i in alive) if term else 0)


def _exact(N, P, board, h, d, k, first=None, seat=0):
    """{winners mask: probability} of a playout to the end under uniform random actions; `first`: the seat's first action"""
    @functools.lru_cache(maxsize=None)
    def rec(board, h, d, k):
        return _dist(board, h, d, k, None)

    def _dist(board, h, d, k, forced):
        alive = [i for i in range(P) if k[i] == 0]
        out = {}
        choices = [(0, 1, -1)] * len(alive)
        joint = [()]
        for ch in choices:
            joint = [j + (a,) for j in joint for a in ch]
        if forced is not None:
            joint = [j for j in joint if j[alive.index(seat)] == forced]
        for j in joint:
            act = [0] * P
            for i, a in zip(alive, j):
                act[i] = a
            nb, nh, nd, nk, term, wm = _py_step(N, P, board, h, d, k, act)
            sub = {wm: 1.0} if term else rec(nb, nh, nd, nk)
            for m, pr in sub.items():
                out[m] = out.get(m, 0.0) + pr / len(joint)
        return out
    return _dist(*(tuple(int(v) for v in t) for t in (board, h, d, k)), first)


def _positions(N, P, B, steps, seed):
    from oracle import oracle as O
    if N == 3:                             # (the reference's layout needs N >= 4: corners, facing each other's column)
        sh, sd = np.array([0, 8], np.int16), np.array([2, 0], np.int8)
    else:
        sh, sd = O.tron_start_positions(N, P)
    st = O.TronState(N, P, B)
    O.tron_reset(st, sh, sd)
    rng = np.random.default_rng(seed)
    for b in range(B):                     # a few random non-terminal moves per game
        one = O.TronState(N, P, 1)
        O.tron_reset(one, sh, sd)
        for _ in range(steps[b]):
            nxt = O.TronState(N, P, 1)
            nxt.board[:], nxt.heads[:], nxt.dirs[:], nxt.deaths[:] = one.board, one.heads, one.dirs, one.deaths
            _, term, _ = O.tron_step(nxt, rng.integers(-1, 2, size=(P, 1)).astype(np.int8))
            if term[0]:
                break
            one = nxt
        st.board[b], st.heads[:, b], st.dirs[:, b], st.deaths[:, b] = one.board[0], one.heads[:, 0], one.dirs[:, 0], one.deaths[:, 0]
    return st


@pytest.mark.parametrize("N", [3, 4])
def test_restatement_matches_exact_probabilities(N):
    P, B, Rn, seed = 2, 3, 2000, 0xBEEF
    st = _positions(N, P, B, [0, 1, 2], seed=N)
    before = (st.board.copy(), st.heads.copy(), st.dirs.copy(), st.deaths.copy())
    cand = np.array([[0, 1, 2]] * B, np.int64)
    wins, played, len_sum, ret_sum = TR.tron_playout(st, seed, Rn, cand=cand, A=3, tcount=np.array([5, 0xFFFFFFFE, 17], np.uint32),
                                                     first_env_id=(1 << 32) + 3)
    assert all(np.array_equal(x, y) for x, y in zip(before, (st.board, st.heads, st.dirs, st.deaths)))   # read only
    assert (played == Rn).all()
    for b in range(B):
        for a in range(3):
            ex = _exact(N, P, st.board[b], st.heads[:, b], st.dirs[:, b], st.deaths[:, b], first=(0, 1, -1)[a])
            for m in range(1 << P):        # winners mask 0 (nobody), 1, 2 (P = 2: both alive is never terminal)
                pq = ex.get(m, 0.0)
                n = int(Rn - wins[b, a].sum()) if m == 0 else int(wins[b, a, m.bit_length() - 1]) if m in (1, 2) else 0
                sigma = math.sqrt(Rn * pq * (1 - pq))
                assert abs(n - Rn * pq) <= 6 * sigma + 1, (N, b, a, m, n, Rn * pq)
            assert Rn <= len_sum[b, a] <= Rn * N * N
            # the seat's return: -1 per step it ends dead, +1 alive, +10 alive at the terminal step
            assert -Rn * N * N <= ret_sum[b, a] <= Rn * (N * N + 10)


def test_restatement_skips_and_stops():
    from oracle import oracle as O
    N, P = 5, 3
    st = _positions(N, P, 4, [0, 0, 0, 0], seed=1)
    st.deaths[1, 1] = 2                    # b = 1: the seat (player 1) is dead
    st.deaths[0, 2] = 1; st.deaths[2, 2] = 3   # b = 2: one player alive
    seat = np.array([0, 1, 1, 3])          # b = 3: seat out of range
    cand = np.array([[0, 3, -1]] * 4)
    wins, played, len_sum, ret_sum = TR.tron_playout(st, 9, 6, cand=cand, A=3, seat=seat)
    assert played.tolist() == [[6, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert (wins[1:] == 0).all() and (len_sum[1:] == 0).all() and (ret_sum[1:] == 0).all() and (len_sum[0, 1:] == 0).all()
    # a cap of one step: every playout is one step; a non-terminal stop counts for nobody
    w1, p1, l1, r1 = TR.tron_playout(st, 9, 6, cand=cand, A=3, seat=seat, max_steps=1)
    assert l1[0, 0] == 6 and (l1[0, 1:] == 0).all() and p1.tolist() == played.tolist()
    assert abs(int(r1[0, 0])) <= 6 * 10 and int(r1[0, 0]) % 2 == 0 or w1[0, 0].sum() > 0
    # P = 1: one terminal step
    one = O.TronState(N, 1, 2)
    sh, sd = O.tron_start_positions(N, 1)
    O.tron_reset(one, sh, sd)
    w, p, l, r = TR.tron_playout(one, 4, 7)
    assert (l == 7).all() and (p == 7).all()
    assert (r[:, 0] == 10 * w[:, 0, 0] - (7 - w[:, 0, 0])).all()
