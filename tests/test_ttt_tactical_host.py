"""TicTacToe's tactical (win-or-block) agent on the host: every argument check of the five C entries (rejected before any
device work), their prototypes and declarations, the Python wrappers' validation and defaults over a stub library, and the
numpy restatement of the contract (tests/ttt_ref.py) on its own -- that the generated positions hold every decision
kind in every row (so the GPU tests cannot be vacuous), the winning cells against a brute force over the line list, the
identities of the contract, and the agent's strength against a uniformly random learner."""
import collections
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import rng_ref as RNG
from tests import ttt_ref as TR
from tests import ttt_probes as TP
from tests.host_util import D, lib as _lib, refused as _refused, ttt_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crl_ttt_winning_cells", "crl_ttt_sample_tactical", "crl_ttt_rollout_tactical", "crl_ttt_step_single_tactical",
           "crl_ttt_playout_tactical")
BAD_NOISE = (-1e-9, math.nextafter(1.0, 2.0), math.nan, math.inf, -math.inf)


@pytest.fixture
def ctx():
    with ttt_context() as h:
        yield _lib(), h


def _common(lib, h, call, name, n_ptr):
    """what all five refuse: a NULL among the first n_ptr pointers, B out of range, no context"""
    for i in range(n_ptr):
        ptrs = [D] * n_ptr
        ptrs[i] = None
        _refused(lib, call(ptrs=ptrs), b"NULL")
    for B in (0, -1, (1 << 31) + 1):
        _refused(lib, call(B=B), b"B=")
    _refused(lib, call(ctx=None), b"tictactoe")
    assert name.encode() in lib.crl_last_error()


def _noise(lib, call):
    for bad in BAD_NOISE:
        _refused(lib, call(noise=bad), b"noise")


def _small_board(lib, call):
    with ttt_context(1, 1, 2, 2, 3) as small:   # fewer cells than players: refused as by crl_ttt_step_single
        _refused(lib, call(ctx=small), b"cells")


def test_winning_cells_argument_checks(ctx):
    lib, h = ctx

    def call(ctx=h, B=4, ptrs=(D, D)):
        return lib.crl_ttt_winning_cells(ctx, B, *ptrs, None)
    _common(lib, h, call, "crl_ttt_winning_cells", 2)


def test_sample_tactical_argument_checks(ctx):
    lib, h = ctx

    def call(ctx=h, B=4, ptrs=(D,) * 4, noise=0.1):
        occ, to_move, tcount, action = ptrs
        return lib.crl_ttt_sample_tactical(ctx, B, 1, 0, occ, to_move, tcount, 1, noise, action, None)
    _common(lib, h, call, "crl_ttt_sample_tactical", 4)
    _noise(lib, call)


def test_rollout_tactical_argument_checks(ctx):
    from colosseumrl_amd import _native
    lib, h = ctx
    fields = [name for name, _ in _native.TTTStats._fields_]

    def call(ctx=h, B=4, ptrs=(D,) * 9, noise=0.1, T=5):
        stats = _native.TTTStats(*[p.value if p is not None else None for p in ptrs[3:]], None)      # (results may be NULL)
        return lib.crl_ttt_rollout_tactical(ctx, B, 1, 0, T, noise, *ptrs[:3], stats, None)
    assert fields[-1] == "results" and len(fields) == 7
    _common(lib, h, call, "crl_ttt_rollout_tactical", 9)
    _noise(lib, call)
    for T in (-1, (1 << 24) + 1):
        _refused(lib, call(T=T), b"T=")
    _refused(lib, call(T=0, noise=2.0), b"noise")          # (checked before the T == 0 early return)


def test_step_single_tactical_argument_checks(ctx):
    lib, h = ctx

    def call(ctx=h, B=4, ptrs=(D,) * 10, noise=0.1, rel_mod=2, flags=0, learner=D):
        occ, winner, to_move, seat, tcount, reward, done, winners, obs, valid = ptrs
        return lib.crl_ttt_step_single_tactical(ctx, B, 1, 0, occ, winner, to_move, seat, learner, tcount, reward, done, winners,
                                                obs, valid, rel_mod, noise, flags, None)
    _common(lib, h, call, "crl_ttt_step_single_tactical", 10)
    _noise(lib, call)
    for flags in (1, 8, 0x80000000):
        _refused(lib, call(flags=flags), b"flags")
    for rel_mod in (0, -2):
        _refused(lib, call(rel_mod=rel_mod), b"rel_mod")
    _refused(lib, call(ptrs=(D,) * 8 + (C.c_void_p(66), D)), b"aligned")
    _small_board(lib, call)


def test_playout_tactical_argument_checks(ctx):
    lib, h = ctx

    def call(ctx=h, B=4, ptrs=(D,) * 6, noise=0.1, cand=D, A=1, Rn=1, flags=0, tcount=D):
        occ, winner, to_move, wins, played, len_sum = ptrs
        return lib.crl_ttt_playout_tactical(ctx, B, 1, 0, occ, winner, to_move, tcount, cand, A, Rn, wins, played, len_sum, noise,
                                            flags, None)
    _common(lib, h, call, "crl_ttt_playout_tactical", 6)
    _noise(lib, call)
    for Rn in (0, -3, 65536):
        _refused(lib, call(Rn=Rn), b"R=")
    for A in (0, -1, 65536):
        _refused(lib, call(A=A), b"A=")
    _refused(lib, call(cand=None, A=2), b"cand")
    for flags in (1, 8, 0x80000000):
        _refused(lib, call(flags=flags), b"flags")
    _small_board(lib, call)


def test_prototypes_and_declarations():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    header = open(os.path.join(ROOT, "include", "colosseum_hip.h")).read()
    common = open(os.path.join(ROOT, "colosseumrl_amd", "csrc", "crl_common.hpp")).read()
    tag, playout_tag = RNG.tag_hex("CRL_TAG_TTT_TACTICAL"), RNG.tag_hex("CRL_TAG_TTT_TACTICAL_PLAYOUT")
    assert "CRL_TAG_TTT_TACTICAL         %su" % tag in common and "CRL_TAG_TTT_TACTICAL_PLAYOUT %su" % playout_tag in common
    assert tag in header and playout_tag in header
    for name in ENTRIES:
        res, args = _native.PROTOTYPES[name]
        assert res is C.c_int and hasattr(_lib(), name)
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, name
        params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):                       # a double exactly where the header has one (noise)
            assert (t is C.c_double) == p.startswith("double "), (name, p)
            assert (t is _native.TTTStats) == p.startswith("crl_ttt_stats "), (name, p)
    sibling = {"crl_ttt_step_single_tactical": "crl_ttt_step_single", "crl_ttt_playout_tactical": "crl_ttt_playout"}
    for name, sib in sibling.items():                        # the sibling's list with `double noise` in front of flags
        args, want = _native.PROTOTYPES[name][1], _native.PROTOTYPES[sib][1]
        assert args[:-3] + args[-2:] == want and args[-3] is C.c_double and args[-2] is C.c_uint32


# ---- the Python wrappers over a stub library (no device: the stream query and the device guard are replaced)
class _StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("crl_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name,) + args)
            return 0
        return entry


class _Guard:
    def __init__(self, dev):
        pass

    def __enter__(self):
        pass

    def __exit__(self, *exc):
        return False


@pytest.fixture
def tb(monkeypatch):
    from colosseumrl_amd import batched
    monkeypatch.setattr(batched, "_stream", lambda: "stream")
    monkeypatch.setattr(batched, "_DevGuard", _Guard)
    monkeypatch.setattr(batched, "_ptr", lambda t: None if t is None else t)       # the tensors themselves, to compare by identity
    obj = batched.TTTBatch.__new__(batched.TTTBatch)
    obj.device, obj.B, obj.P, obj.n_cells, obj.first_env_id = torch.device("cpu"), 5, 2, 9, 40
    obj._lib, obj._ctx = _StubLib(), types.SimpleNamespace(handle="handle")
    for k, (dt, shape) in {**batched.TTTBatch._stat_spec(5, 2), "occ": (torch.int32, (2, 5)), "winner": (torch.int8, (5,)),
                           "to_move": (torch.int8, (5,)), "reward": (torch.int8, (5,)), "winners": (torch.int8, (5,))}.items():
        setattr(obj, k, torch.zeros(shape, dtype=dt))
    return obj


def test_wrapper_defaults_are_the_existing_entries(tb):
    seat, act = torch.zeros(5, dtype=torch.int8), torch.zeros(5, dtype=torch.int64)
    cand = torch.zeros((5, 3), dtype=torch.int32)
    out = tb.step_single(seat, act, 7)
    po = tb.playout(4, cand, 8)
    tb.flat_mc_action(2, 9)
    calls = tb._lib.calls
    assert [c[0] for c in calls] == ["crl_ttt_step_single", "crl_ttt_playout", "crl_ttt_playout"]
    assert calls[0][1:] == ("handle", 5, 7, 40, tb.occ, tb.winner, tb.to_move, seat, act, tb.tcount, tb.reward, out["done"],
                            tb.winners, out["board"], out["valid"], 2, 0, "stream")
    assert calls[1][1:] == ("handle", 5, 8, 40, tb.occ, tb.winner, tb.to_move, tb.tcount, cand, 3, 4, po["wins"], po["played"],
                            po["len_sum"], 0, "stream")
    assert calls[2][9:12] == (tb._all_cells, 9, 2) and calls[2][-2:] == (0, "stream")
    tb._lib.calls = []
    tb.step_single(seat, act, 7, opponent="random", noise=0.9)     # the noise of a random opponent goes nowhere
    tb.playout(4, cand, 8, agent="random", noise=0.9)
    assert [c[0] for c in tb._lib.calls] == ["crl_ttt_step_single", "crl_ttt_playout"]
    assert tb._lib.calls[0][-2:] == (0, "stream") and tb._lib.calls[1][-2:] == (0, "stream")


def test_wrapper_tactical_calls(tb):
    seat, act = torch.zeros(5, dtype=torch.int8), torch.zeros(5, dtype=torch.int64)
    cand = torch.zeros((5, 3), dtype=torch.int32)
    cells = tb.winning_cells()
    a1 = tb.sample_tactical(3)
    tb.sample_tactical(3, 0.25, advance=False)
    tb.rollout_tactical(6, 4)
    out = tb.step_single(seat, None, 7, opponent="tactical")
    po = tb.playout(4, cand, 8, agent="tactical", noise=1)
    tb.flat_mc_action(2, 9, agent="tactical", noise=0.5)
    c = tb._lib.calls
    assert [x[0] for x in c] == ["crl_ttt_winning_cells", "crl_ttt_sample_tactical", "crl_ttt_sample_tactical",
                                 "crl_ttt_rollout_tactical", "crl_ttt_step_single_tactical", "crl_ttt_playout_tactical",
                                 "crl_ttt_playout_tactical"]
    assert c[0][1:] == ("handle", 5, tb.occ, cells, "stream") and cells.dtype == torch.int32 and tuple(cells.shape) == (2, 5)
    assert c[1][1:] == ("handle", 5, 3, 40, tb.occ, tb.to_move, tb.tcount, 1, 0.1, a1, "stream") and a1.dtype == torch.int8
    assert c[2][8:10] == (0, 0.25)
    assert c[3][1:7] == ("handle", 5, 4, 40, 6, 0.1) and c[3][7:10] == (tb.occ, tb.winner, tb.to_move)
    assert isinstance(c[3][10], type(tb._stats())) and c[3][10].tcount == tb.tcount.data_ptr() and c[3][11] == "stream"
    assert c[4][1:] == ("handle", 5, 7, 40, tb.occ, tb.winner, tb.to_move, seat, None, tb.tcount, tb.reward, out["done"],
                        tb.winners, out["board"], out["valid"], 2, 0.1, 0, "stream")
    assert c[5][1:] == ("handle", 5, 8, 40, tb.occ, tb.winner, tb.to_move, tb.tcount, cand, 3, 4, po["wins"], po["played"],
                        po["len_sum"], 1.0, 0, "stream") and isinstance(c[5][-3], float)
    assert c[6][-3:] == (0.5, 0, "stream")


def test_wrapper_validation(tb):
    seat, act = torch.zeros(5, dtype=torch.int8), torch.zeros(5, dtype=torch.int64)
    for bad in ("avoid", "Tactical", None, 1):
        with pytest.raises(ValueError, match="opponent"):
            tb.step_single(seat, act, opponent=bad)
        with pytest.raises(ValueError, match="agent"):
            tb.playout(3, agent=bad)
        with pytest.raises(ValueError, match="agent"):
            tb.flat_mc_action(3, agent=bad)
    for bad in BAD_NOISE + ("0.1", True, None):
        for call in (lambda: tb.sample_tactical(1, bad), lambda: tb.rollout_tactical(3, 1, bad),
                     lambda: tb.step_single(seat, act, noise=bad), lambda: tb.step_single(seat, act, opponent="tactical", noise=bad),
                     lambda: tb.playout(3, noise=bad), lambda: tb.flat_mc_action(3, agent="tactical", noise=bad)):
            with pytest.raises(ValueError, match="noise"):
                call()
    assert tb._lib.calls == []


def test_vector_env_validation(monkeypatch):
    from colosseumrl_amd import _native
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    monkeypatch.setattr(_native, "require_gpu", lambda: pytest.fail("validated before any native call"))
    with pytest.raises(ValueError, match="opponent"):
        TicTacToeSinglePlayerVectorEnv(batch=8, opponent="avoid")
    for bad in (-0.1, 1.5, math.nan, "x"):
        with pytest.raises(ValueError, match="noise"):
            TicTacToeSinglePlayerVectorEnv(batch=8, opponent="tactical", noise=bad)


# ---- the restatement on its own
def _popcounts(a):
    return np.array([bin(int(x)).count("1") for x in a])


_MULTI_ROWS = {}


@pytest.mark.parametrize("cfg", TP.INSTANCE_ROWS, ids=TP.INSTANCE_IDS)
def test_positions_hold_every_decision_kind(cfg):
    st = TR.state_of(cfg)
    assert st.B == 203
    kinds, S, E = TR.kinds(st)
    count = collections.Counter(kinds)
    want = [TR.OWN, TR.NONE, TR.OVER] + ([TR.NEXT] if cfg[2] >= 2 else []) + ([TR.LATER] if cfg[2] >= 3 else [])
    for kind in want:
        assert count[kind] >= 8, (kind, dict(count))
    assert set(count) == set(want)
    _MULTI_ROWS[cfg] = bool(((_popcounts(S) > 1) & (_popcounts(S) < _popcounts(E))).any())
    small = collections.Counter(TR.kinds(TR.state_of(cfg, 37))[0])    # the 37 of the rollout and single-step tests
    assert all(small[kind] >= 1 for kind in want), dict(small)
    assert {0, 1, 2 ** 32 - 1} <= set(int(c) for c in st.tcount)


def test_enough_rows_choose_among_several_cells():
    for cfg in TP.INSTANCE_ROWS:                                     # (also when this test runs alone)
        if cfg not in _MULTI_ROWS:
            _, S, E = TR.kinds(TR.state_of(cfg))
            _MULTI_ROWS[cfg] = bool(((_popcounts(S) > 1) & (_popcounts(S) < _popcounts(E))).any())
    assert sum(_MULTI_ROWS.values()) >= 12, _MULTI_ROWS


@pytest.mark.parametrize("cfg", [((3, 3), 3, 2), ((2, 8), 5, 5), ((32,), 7, 7), ((3, 3, 3), 2, 6), ((4, 7), 4, 8)],
                         ids=["3x3k3p2", "2x8k5p5", "32k7p7", "3x3x3k2p6", "4x7k4p8"])
def test_winning_cells_against_the_line_list(cfg):
    """W_q by the definition over TP.line_masks (walked coordinates): has_line's array slices are not involved"""
    dims, K, P = cfg
    st = TR.state_of(cfg)
    lines = [int(m) for m in TP.line_masks(dims, K)]
    got = TR.winning_cells(st)
    E = TR.empties(dims, st.occ)
    for b in range(st.B):
        for q in range(P):
            want = 0
            for e in range(st.n_cells):
                mm = int(st.occ[q, b]) | (1 << e)
                if (int(E[b]) >> e) & 1 and any((mm & ln) == ln for ln in lines):
                    want |= 1 << e
            assert int(got[q, b]) == want, (b, q)


def test_threshold():
    assert RNG.threshold(0.0) == 0 and RNG.threshold(1.0) == 1 << 32 and RNG.threshold(0.5) == 1 << 31
    assert RNG.threshold(2.0 ** -33) == 1 and RNG.threshold(1.0 - 2.0 ** -40) == 1 << 32


@pytest.mark.parametrize("cfg", [((3, 5), 3, 3), ((4, 4), 4, 4), ((2, 2, 8), 2, 5)], ids=["3x5k3p3", "4x4k4p4", "2x2x8k2p5"])
def test_the_move_follows_the_contract(cfg):
    dims, K, P = cfg
    st = TR.state_of(cfg)
    W = TR.winning_cells(st)
    E = TR.empties(dims, st.occ)
    quiet, loud = TR.sample(st, 5, TR.tactical_agent(0.0), advance=False), TR.sample(st, 5, TR.tactical_agent(1.0), advance=False)
    some = TR.sample(st, 5, TR.tactical_agent(0.1), advance=False)
    assert (st.tcount == TR.positions(cfg)["tcount"]).all()        # advance=False
    n_noisy = 0
    for b in range(st.B):
        tm = int(st.to_move[b])
        if int(E[b]) == 0:
            assert quiet[b] == loud[b] == some[b] == -1
            continue
        assert (int(E[b]) >> int(loud[b])) & 1 and (int(E[b]) >> int(quiet[b])) & 1
        order = [int(W[(tm + i) % P, b]) for i in range(P)]
        first = next((w for w in order if w), int(E[b]))
        assert (first >> int(quiet[b])) & 1, b                   # its own win, else the earliest threat, else any empty cell
        assert some[b] in (quiet[b], loud[b])                    # one draw: the noise only chooses the set
        n_noisy += some[b] != quiet[b]
    assert 0 < n_noisy < 60                                      # about a tenth of the plies, fewer where the sets agree
    before = st.tcount.copy()
    TR.sample(st, 5, TR.tactical_agent(0.1))
    assert (st.tcount == before + np.uint32(1)).all()              # advance (2^32 - 1 wraps to 0)


@pytest.mark.parametrize("cfg", [((3, 3), 3, 2), ((3, 5), 3, 3)], ids=["3x3k3p2", "3x5k3p3"])
def test_a_learner_that_plays_the_agents_move_is_the_rollout(cfg):
    from oracle import oracle as O
    dims, K, P = cfg
    B, seed, noise = 24, 31, 0.1
    st = O.TTTState(dims, K, P, B)
    seat = (np.arange(B) % P).astype(np.int8)

    def policy(s):
        return TR.sample(s, seed, TR.tactical_agent(noise), advance=False).astype(np.int64)
    TR.step_single(st, seat, None, seed, TR.tactical_agent(noise))
    n_done = 0
    for _ in range(8):
        n_done += int(TR.step_single(st, seat, None, seed, TR.tactical_agent(noise), policy=policy)[1].sum())
    assert n_done > 0 and (st.to_move == seat).all()
    for g in range(B):
        ref = O.TTTState(dims, K, P, 1)
        TR.rollout(ref, seed, TR.tactical_agent(noise), int(st.tcount[g]), first_env_id=g)
        assert np.array_equal(ref.occ[:, 0], st.occ[:, g]) and ref.winner[0] == st.winner[g] and ref.to_move[0] == st.to_move[g], g


def test_playout_without_a_candidate_is_the_rollouts_first_episode():
    """row (b, 0) of a playout with cand == NULL and R = 1 ... under the playout's own tag: the same plies as sample-and-step
    with the third counter word and tag of the playout, stopped at the first terminal ply"""
    from oracle import oracle as O
    cfg = ((3, 5), 3, 3)
    st = TR.state_of(cfg, 37)
    wins, played, len_sum = TR.playout(st, 9, 3, TR.tactical_agent(0.1), first_env_id=100, tcount=st.tcount)
    over = (st.winner >= 0) | (TR.empties(cfg[0], st.occ) == 0)
    assert (played[~over, 0] == 3).all() and not played[over].any() and not len_sum[over].any() and not wins[over].any()
    for b in np.flatnonzero(~over)[:10]:
        for r in range(3):
            one = O.TTTState(*cfg, 1)
            one.occ[:, 0], one.to_move[0] = st.occ[:, b], st.to_move[b]
            c, plies = int(st.tcount[b]), 0
            while True:
                u, v = TR.draws(9, [100 + b], [c], [r], RNG.CRL_TAG_TTT_TACTICAL_PLAYOUT)
                act, _, _ = TR.moves(cfg[0], cfg[1], cfg[2], one.occ, one.to_move, u, v, 0.1)
                _, term, ws = O.ttt_step(one, act)
                plies, c = plies + 1, (c + 1) & 0xFFFFFFFF
                if term[0]:
                    break
            len_sum[b, 0] -= plies
            if ws[0] >= 0:
                wins[b, 0, ws[0]] -= 1
    assert not len_sum[np.flatnonzero(~over)[:10]].any() and not wins[np.flatnonzero(~over)[:10]].any()


def _uniform_learner_share(step, B, rng):
    """the win share among finished games of a learner that plays a uniformly random empty cell at seat 0 of 3x3, until
    every game has finished at least once; step(actions or None) -> (reward, done, valid)"""
    _, _, valid = step(None)
    seen = np.zeros(B, bool)
    wins = finished = 0
    for _ in range(5):
        free = ((valid[:, None] >> np.arange(9, dtype=np.uint32)[None, :]) & 1).astype(bool)
        act = np.where(free, rng.random((B, 9)), -1.0).argmax(axis=1).astype(np.int64)
        reward, done, valid = step(act)
        wins += int(((done != 0) & (reward == 1)).sum())
        finished += int((done != 0).sum())
        seen |= done != 0
    assert seen.all()
    return wins / finished


def test_strength_on_the_restatement():
    """the condition of the GPU strength test at B = 1024 (binomial deviation 0.016): at least 0.45 against the random agent
    (the restatement of crl_ttt_step_single), at most 0.15 against the noise-free tactical one"""
    from oracle import oracle as O
    B, seat = 1024, np.zeros(1024, np.int8)
    st = O.TTTState((3, 3), 3, 2, B)

    def against_random(act):
        reward, done, _, _, valid = TR.step_single(st, seat, act, 2024, TR.random_agent)
        return reward, done, valid
    rnd = _uniform_learner_share(against_random, B, np.random.default_rng(1))
    st = O.TTTState((3, 3), 3, 2, B)

    def against_tactical(act):
        reward, done, _, _, valid = TR.step_single(st, seat, act, 2024, TR.tactical_agent(0.0))
        return reward, done, valid
    tac = _uniform_learner_share(against_tactical, B, np.random.default_rng(1))
    assert rnd >= 0.45 and tac <= 0.15, (rnd, tac)
