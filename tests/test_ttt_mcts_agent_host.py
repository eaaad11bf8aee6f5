"""The tree search as a seated agent (crl_ttt_sample_mcts / _rollout_mcts / _step_single_mcts) on the host: every refusal of
the three C entries with its message (on dummy pointers, before any device work), their prototypes and declarations under
the unchanged revision, the Python wrappers' validation and exact native-call argument tuples over a stub library, and the
restatement of the contract (tests/mcts_agent_ref.py) on its own -- at noise 1 the tactical agent's moves, at noise 0 the
search's `best`, and its strength as an opponent next to the tactical agent."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import mcts_agent_ref as AR
from tests import mcts_ref as M
from tests import ttt_ref as TR
from tests.host_util import D, lib as _lib, refused as _refused, tron_context, ttt_context
from tests.test_ttt_tactical_host import tb  # noqa: F401  (the fixture: a TTTBatch over a stub library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crl_ttt_sample_mcts", "crl_ttt_rollout_mcts", "crl_ttt_step_single_mcts")
BAD_NOISE = (-1e-9, math.nextafter(1.0, 2.0), math.nan, math.inf, -math.inf)
S_MAX_3X3 = 2519


@pytest.fixture
def ctx():
    with ttt_context() as h:
        yield _lib(), h


def _common(lib, h, call, name, n_ptr):
    """what all three refuse: a NULL among the first n_ptr pointers, B out of range, no context or another game's, and the
    search's and the noise's limits"""
    for i in range(n_ptr):
        ptrs = [D] * n_ptr
        ptrs[i] = None
        _refused(lib, call(ptrs=ptrs), b"NULL", name.encode())
    for B in (0, -1, (1 << 31) + 1):
        _refused(lib, call(B=B), b"B=", name.encode())
    _refused(lib, call(ctx=None), b"tictactoe", name.encode())
    with tron_context() as tron:
        _refused(lib, call(ctx=tron), b"tictactoe")
    for S in (0, -1, S_MAX_3X3 + 1, 4096, 1 << 30):
        _refused(lib, call(S=S), b"S=", b"1..2519", name.encode())
    for Rn in (0, -3, 1025, 65535):
        _refused(lib, call(Rn=Rn), b"R=", name.encode())
    for cexp in (65536, 0xFFFFFFFF):
        _refused(lib, call(cexp=cexp), b"cexp=", name.encode())
    for bad in BAD_NOISE:
        _refused(lib, call(noise=bad), b"noise", name.encode())


def test_sample_mcts_argument_checks(ctx):
    lib, h = ctx

    def call(ctx=h, B=4, ptrs=(D,) * 4, S=8, Rn=4, cexp=256, noise=0.0):
        occ, to_move, tcount, action = ptrs
        return lib.crl_ttt_sample_mcts(ctx, B, 1, 0, occ, to_move, tcount, 1, S, Rn, cexp, noise, action, None)
    _common(lib, h, call, "crl_ttt_sample_mcts", 4)


def test_rollout_mcts_argument_checks(ctx):
    from colosseumrl_amd import _native
    lib, h = ctx

    def call(ctx=h, B=4, ptrs=(D,) * 9, S=8, Rn=4, cexp=256, noise=0.0, T=5):
        stats = _native.TTTStats(*[p.value if p is not None else None for p in ptrs[3:]], None)      # (results may be NULL)
        return lib.crl_ttt_rollout_mcts(ctx, B, 1, 0, T, S, Rn, cexp, noise, *ptrs[:3], stats, None)
    _common(lib, h, call, "crl_ttt_rollout_mcts", 9)
    for T in (-1, (1 << 24) + 1):
        _refused(lib, call(T=T), b"T=")
    _refused(lib, call(T=0, noise=2.0), b"noise")          # (checked before the T == 0 early return, as the tactical sibling)
    _refused(lib, call(T=0, S=0), b"S=")
    assert call(T=0) == 0                                  # T = 0 launches nothing


def test_step_single_mcts_argument_checks(ctx):
    lib, h = ctx

    def call(ctx=h, B=4, ptrs=(D,) * 10, S=8, Rn=4, cexp=256, noise=0.0, rel_mod=2, flags=0, learner=D):
        occ, winner, to_move, seat, tcount, reward, done, winners, obs, valid = ptrs
        return lib.crl_ttt_step_single_mcts(ctx, B, 1, 0, occ, winner, to_move, seat, learner, tcount, reward, done, winners, obs,
                                            valid, rel_mod, S, Rn, cexp, noise, flags, None)
    _common(lib, h, call, "crl_ttt_step_single_mcts", 10)
    for flags in (1, 8, 0x80000000):
        _refused(lib, call(flags=flags), b"flags")
    for rel_mod in (0, -2):
        _refused(lib, call(rel_mod=rel_mod), b"rel_mod")
    _refused(lib, call(ptrs=(D,) * 8 + (C.c_void_p(66), D)), b"aligned")
    with ttt_context(1, 1, 2, 2, 3) as small:              # fewer cells than players: refused as by crl_ttt_step_single
        _refused(lib, call(ctx=small), b"cells")


@pytest.mark.parametrize("d, k, p, s_max", [((1, 3, 5), 3, 3, 1723), ((3, 3, 3), 3, 4, 1056), ((1, 4, 8), 4, 2, 909)],
                         ids=["3x5", "3x3x3", "4x8"])
def test_s_max_is_the_searchs(d, k, p, s_max):
    """S_max passes the check of S, S_max + 1 does not, and crl_ttt_mcts_max_simulations is unchanged (the calls with S_max are
    stopped by a later check, so that nothing is launched on the dummy pointers)"""
    lib = _lib()
    with ttt_context(*d, k, p) as h:
        assert lib.crl_ttt_mcts_max_simulations(h) == s_max == M.max_simulations(d[0] * d[1] * d[2])
        for S, word in ((s_max, b"noise"), (s_max + 1, b"S=")):
            _refused(lib, lib.crl_ttt_sample_mcts(h, 4, 1, 0, D, D, D, 1, S, 4, 256, 2.0, D, None), word)
            _refused(lib, lib.crl_ttt_step_single_mcts(h, 4, 1, 0, *[D] * 11, p, S, 4, 256, 2.0, 0, None), word)


def test_prototypes_and_declarations():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    header = open(os.path.join(ROOT, "include", "colosseum_hip.h")).read()
    for name in ENTRIES:
        res, args = _native.PROTOTYPES[name]
        assert res is C.c_int and hasattr(_lib(), name)
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, name
        params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):
            assert (t is C.c_double) == p.startswith("double "), (name, p)
            assert (t is _native.TTTStats) == p.startswith("crl_ttt_stats "), (name, p)
            assert (t is C.c_uint32) == (p.startswith("uint32_t ") and "*" not in p), (name, p)
            assert (t is C.c_int) == p.startswith("int "), (name, p)
    # the tactical sibling's list with `int S, int R, uint32_t cexp` in front of `double noise`
    search = [C.c_int, C.c_int, C.c_uint32]
    for name in ENTRIES:
        args, want = _native.PROTOTYPES[name][1], _native.PROTOTYPES[name.replace("_mcts", "_tactical")][1]
        at = args.index(C.c_double)
        assert args[at - 3:at] == search and args[:at - 3] + args[at:] == want, name


# ---- the Python wrappers over a stub library
def test_wrapper_calls(tb):  # noqa: F811
    tb.__dict__["mcts_max_simulations"] = S_MAX_3X3
    seat, act = torch.zeros(5, dtype=torch.int8), torch.zeros(5, dtype=torch.int64)
    a1 = tb.sample_mcts(24)
    tb.sample_mcts(30, 8, 3, 0.5, 0.25, advance=False)
    tb.rollout_mcts(6, 24)
    tb.rollout_mcts(7, 40, 2, 4, 2.0, 1)
    out = tb.step_single(seat, None, 7, opponent="mcts", simulations=24)
    tb.step_single(seat, act, 7, 3, out, "mcts", 0.5, 40, 2, 0.25)
    c = tb._lib.calls
    assert [x[0] for x in c] == ["crl_ttt_sample_mcts"] * 2 + ["crl_ttt_rollout_mcts"] * 2 + ["crl_ttt_step_single_mcts"] * 2
    assert c[0][1:] == ("handle", 5, 0, 40, tb.occ, tb.to_move, tb.tcount, 1, 24, 16, 256, 0.0, a1, "stream")
    assert a1.dtype == torch.int8 and tuple(a1.shape) == (5,) and isinstance(c[0][12], float)
    assert c[1][1:13] == ("handle", 5, 3, 40, tb.occ, tb.to_move, tb.tcount, 0, 30, 8, 128, 0.25)
    assert c[2][1:10] == ("handle", 5, 0, 40, 6, 24, 16, 256, 0.0) and c[2][10:13] == (tb.occ, tb.winner, tb.to_move)
    assert isinstance(c[2][13], type(tb._stats())) and c[2][13].tcount == tb.tcount.data_ptr() and c[2][14] == "stream"
    assert c[3][1:10] == ("handle", 5, 4, 40, 7, 40, 2, 512, 1.0) and isinstance(c[3][9], float)
    assert c[4][1:] == ("handle", 5, 7, 40, tb.occ, tb.winner, tb.to_move, seat, None, tb.tcount, tb.reward, out["done"],
                        tb.winners, out["board"], out["valid"], 2, 24, 16, 256, 0.1, 0, "stream")
    assert c[5][1:] == ("handle", 5, 7, 40, tb.occ, tb.winner, tb.to_move, seat, act, tb.tcount, tb.reward, out["done"],
                        tb.winners, out["board"], out["valid"], 3, 40, 2, 64, 0.5, 0, "stream")
    tb._lib.calls = []                                      # the search's keywords go nowhere with the other opponents
    tb.step_single(seat, act, 7, opponent="random", simulations=24)
    tb.step_single(seat, act, 7, opponent="tactical", noise=0.3, simulations=24, playouts=3, exploration=2.0)
    assert tb._lib.calls[0][0] == "crl_ttt_step_single" and tb._lib.calls[0][-3:] == (2, 0, "stream")
    assert tb._lib.calls[1][0] == "crl_ttt_step_single_tactical" and tb._lib.calls[1][-4:] == (2, 0.3, 0, "stream")


def test_wrapper_validation(tb):  # noqa: F811
    from colosseumrl_amd.batched import TTTBatch
    tb.__dict__["mcts_max_simulations"] = S_MAX_3X3
    seat, act = torch.zeros(5, dtype=torch.int8), torch.zeros(5, dtype=torch.int64)
    calls = {"sample": lambda **kw: tb.sample_mcts(**{"simulations": 8, **kw}),
             "rollout": lambda **kw: tb.rollout_mcts(3, **{"simulations": 8, **kw}),
             "single": lambda **kw: tb.step_single(seat, act, opponent="mcts", **{"simulations": 8, **kw})}
    for name, call in calls.items():
        for bad in (0, S_MAX_3X3 + 1, -1, 2.0, True, "8"):
            with pytest.raises(ValueError, match="simulations"):
                call(simulations=bad)
        for bad in (0, 1025, 16.0, False, None):
            with pytest.raises(ValueError, match="playouts"):
                call(playouts=bad)
        for bad in (-0.5, 256.0, float("nan"), "1", True, None):
            with pytest.raises(ValueError, match="exploration"):
                call(exploration=bad)
        for bad in BAD_NOISE + ("0.1", True, None):
            with pytest.raises(ValueError, match="noise"):
                call(noise=bad)
    with pytest.raises(ValueError, match="simulations"):
        tb.step_single(seat, act, opponent="mcts")          # no default budget for an opponent
    with pytest.raises(ValueError, match="simulations"):
        tb.step_single(seat, act, opponent="mcts", simulations=None)
    assert TTTBatch.AGENTS == ("random", "tactical") and TTTBatch.OPPONENTS == ("random", "tactical", "mcts")
    for fn in (tb.playout, tb.flat_mc_action):              # the playout policies stay the two scripted agents
        with pytest.raises(ValueError, match="agent"):
            fn(3, agent="mcts")
    with pytest.raises(ValueError, match="opponent"):
        tb.step_single(seat, act, opponent="MCTS", simulations=8)
    assert tb._lib.calls == []


def test_vector_env_validation(monkeypatch):
    from colosseumrl_amd import _native
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    monkeypatch.setattr(_native, "require_gpu", lambda: pytest.fail("validated before any native call"))
    with pytest.raises(ValueError, match="opponent"):
        TicTacToeSinglePlayerVectorEnv(batch=8, opponent="search")
    for kw, word in ((dict(simulations=0), "simulations"), (dict(simulations=S_MAX_3X3 + 1), "simulations"),
                     (dict(simulations=1724, dims=(3, 5)), "simulations"), (dict(simulations=8.0), "simulations"),
                     (dict(playouts=0), "playouts"), (dict(playouts=1025), "playouts"), (dict(exploration=-1.0), "exploration"),
                     (dict(exploration=math.nan), "exploration"), (dict(noise=1.5), "noise"), (dict(noise=math.nan), "noise")):
        with pytest.raises(ValueError, match=word):
            TicTacToeSinglePlayerVectorEnv(batch=8, opponent="mcts", **kw)


# ---- the restatement on its own
def test_noise_one_is_the_tactical_agent_at_noise_one():
    for cfg in (((3, 3), 3, 2), ((3, 5), 3, 3), ((3, 3, 3), 3, 4)):
        st = TR.state_of(cfg)                                # 203 positions: full boards and every counter parity among them
        want = TR.sample(st, 5, TR.tactical_agent(1.0), 9, advance=False)
        got = TR.sample(st, 5, AR.mcts_agent(7, 2, 256, 1.0), 9, advance=False)
        assert np.array_equal(got, want) and (want == -1).any() and (want >= 0).sum() > 150


def test_noise_zero_is_the_searchs_best():
    rng = np.random.default_rng(4)
    for dims, K, P in (((3, 3), 3, 2), ((3, 5), 3, 3)):
        st = M.positions(dims, K, P, 24, rng)               # finished positions and movers out of range among them
        count = {}
        got = TR.sample(st, 6, AR.mcts_agent(20, 3, 300, 0.0, count), 77, advance=False)
        best = M.ttt_mcts(st, 20, 3, 300, 6, 77, st.tcount)[3]
        E = TR.empties(dims, st.occ)
        out_of_range = (st.to_move < 0) | (st.to_move >= P)
        searched = ~out_of_range & (E != 0)
        # the agent reads occ and to_move only: a recorded winner does not stop it, crl_ttt_mcts skips that position
        plain = searched & (st.winner < 0)
        assert np.array_equal(got[plain], best[plain]) and plain.sum() >= 12 and count["searches"] == searched.sum()
        assert (got[~searched] == -1).all() and (~searched).sum() >= 3 and (got[searched] >= 0).all()
        assert all((int(E[b]) >> int(got[b])) & 1 for b in np.flatnonzero(searched))


def test_some_noise_mixes_the_two():
    st = M.positions((3, 3), 3, 2, 40, np.random.default_rng(8), plant=False)
    quiet = TR.sample(st, 3, AR.mcts_agent(12, 2, 256, 0.0), advance=False)
    loud = TR.sample(st, 3, AR.mcts_agent(12, 2, 256, 1.0), advance=False)
    count = {}
    some = TR.sample(st, 3, AR.mcts_agent(12, 2, 256, 0.3, count), advance=False)
    u, _ = TR.draws(3, np.arange(40), st.tcount)
    noisy = u < np.uint64(math.ceil(0.3 * 2 ** 32))
    assert np.array_equal(some, np.where(noisy, loud, quiet)) and 4 <= noisy.sum() <= 22 and count["searches"] == (~noisy).sum()


# ---- strength: a uniformly random learner at seat 0 of 3x3, first episodes
def _first_episode_wins(agent, games, seed):
    """how many of `games` first episodes the uniformly random learner at seat 0 wins against `agent` at seat 1"""
    from oracle import oracle as O
    st, seat = O.TTTState((3, 3), 3, 2, games), np.zeros(games, np.int8)
    rng = np.random.default_rng(seed)
    valid = TR.step_single(st, seat, None, seed, agent)[4]
    live, wins = np.ones(games, bool), 0
    for _ in range(5):                                       # the learner has at most five plies in a game
        free = ((valid[:, None] >> np.arange(9, dtype=np.uint32)[None, :]) & 1).astype(bool)
        act = np.where(free, rng.random((games, 9)), -1.0).argmax(axis=1).astype(np.int64)
        reward, done, _, _, valid = TR.step_single(st, seat, act, seed, agent)
        wins += int((live & (done != 0) & (reward == 1)).sum())
        live &= done == 0
    assert not live.any()
    return wins


def test_the_search_opponent_is_at_least_twice_as_hard_as_the_tactical_one():
    """3x3, 200 first episodes, seed 11: the learner wins at most half as often against the noise-free search opponent (64
    simulations x 16 playouts, exploration 1.0) as against the noise-free tactical agent, and the latter count is above 0.
    The same condition as the GPU test's (tests/test_gpu_ttt_mcts_agent.py)."""
    games, seed = 200, 11
    tactical = _first_episode_wins(TR.tactical_agent(0.0), games, seed)
    search = _first_episode_wins(AR.mcts_agent(64, 16, 256, 0.0), games, seed)
    print("learner wins of %d first episodes: against tactical %d, against the search %d" % (games, tactical, search))
    assert tactical > 0 and 2 * search <= tactical, (search, tactical)
