"""The territory tree search as a seated agent (crl_tron_sample_mcts_territory, crl_tron_sample_mcts_territory_max_simulations)
on the host: every refusal of the two C entries with the argument named, S_agent against the restatement, the prototypes, the
argument checks of the Python wrappers, the plain-Python restatement of the contract (tests/tron_mcts_agent_ref.py) held to
the two contracts it is made of, and the shape list of the GPU tests against the kernel's template instances."""
import itertools

import numpy as np
import pytest

from tests import territory_ref as TV
from tests import tron_mcts_agent_ref as A
from tests import tron_mcts_ref as M
from tests import tron_mcts_territory_ref as T
from tests.host_util import D, fake as _fake, lib as _lib, tron_context, ttt_context

SIZES = (5, 19, 20, 40, 64)


def _call(lib, ctx, B=4, tcount=D, advance=1, noise=0.1, mask=1, state=(D,) * 4, S=8, V=256, cexp=256, model_noise=0.1, flags=0,
          actions=D):
    return lib.crl_tron_sample_mcts_territory(ctx, B, 1, 0, tcount, advance, noise, mask, *state, S, V, cexp, model_noise, flags,
                                              actions, None)


def _layout(N, P):
    """a start layout for a context: P distinct cells, everybody heading east"""
    return tuple(range(0, 2 * P, 2)), (1,) * P


def test_argument_checks():
    lib = _lib()
    with tron_context(5, 3, *_layout(5, 3)) as h, ttt_context() as tt:
        name = b"crl_tron_sample_mcts_territory: "
        for i in range(4):                 # board, heads, dirs, deaths
            st = [D] * 4
            st[i] = None
            assert _call(lib, h, state=tuple(st)) == -1 and name + b"NULL state" in lib.crl_last_error()
        assert _call(lib, h, tcount=None) == -1 and name + b"NULL tcount" in lib.crl_last_error()
        assert _call(lib, h, actions=None) == -1 and name + b"NULL tcount / actions" in lib.crl_last_error()
        for B in (0, -1, (1 << 31) + 1):
            assert _call(lib, h, B=B) == -1 and name + b"B=" in lib.crl_last_error()
        for mask in (0, 8, 9, 0x80000000):                       # empty, or a bit at P = 3 and beyond
            assert _call(lib, h, mask=mask) == -1 and name + b"player_mask" in lib.crl_last_error()
        for noise in (-0.01, 1.0001, float("nan"), float("inf")):
            assert _call(lib, h, noise=noise) == -1 and name + b"noise=" in lib.crl_last_error()
            assert _call(lib, h, model_noise=noise) == -1 and name + b"model_noise=" in lib.crl_last_error()
        for mask in (1, 3, 7):
            s_agent = lib.crl_tron_sample_mcts_territory_max_simulations(h, mask)
            assert s_agent == A.agent_max_simulations(5, bin(mask).count("1"))
            for S in (0, s_agent + 1, -1, 4096):
                assert _call(lib, h, mask=mask, S=S) == -1 and name + b"S=" in lib.crl_last_error()
            # the largest arguments pass every check before the flags (nothing is launched on the dummy pointers)
            assert _call(lib, h, mask=mask, S=s_agent, V=1024, cexp=65535, noise=1.0, model_noise=1.0, flags=2) == -1
            assert name + b"unknown flags" in lib.crl_last_error()
        for V in (0, 1025, -1):
            assert _call(lib, h, V=V) == -1 and name + b"V=" in lib.crl_last_error()
        for cexp in (65536, 0xFFFFFFFF):
            assert _call(lib, h, cexp=cexp) == -1 and name + b"cexp=" in lib.crl_last_error()
        for flags in (2, 3, 4, 0x80000000):           # CRL_PLAYOUT_AVOID (1) only
            assert _call(lib, h, flags=flags) == -1 and name + b"unknown flags" in lib.crl_last_error()
        assert _call(lib, h, S=1, V=1, cexp=0, noise=0.0, model_noise=0.0, advance=0, flags=2) == -1 and b"flags" in lib.crl_last_error()
        assert _call(lib, None) == -1 and name + b"ctx is not a tron context" in lib.crl_last_error()
        assert _call(lib, tt) == -1 and name + b"ctx is not a tron context" in lib.crl_last_error()


def test_max_simulations_argument_checks():
    lib = _lib()
    name = b"crl_tron_sample_mcts_territory_max_simulations: "
    with tron_context(5, 3, *_layout(5, 3)) as h, ttt_context() as tt:
        for mask in (0, 8, 15, 0x80000000):
            assert lib.crl_tron_sample_mcts_territory_max_simulations(h, mask) == -1 and name + b"player_mask" in lib.crl_last_error()
        assert lib.crl_tron_sample_mcts_territory_max_simulations(None, 1) == -1 and name + b"ctx is not a tron context" in lib.crl_last_error()
        assert lib.crl_tron_sample_mcts_territory_max_simulations(tt, 1) == -1 and name + b"ctx is not a tron context" in lib.crl_last_error()


@pytest.mark.parametrize("N", [65, 89, 181])
def test_boards_wider_than_64_are_unsupported(N):
    lib = _lib()
    with tron_context(N, 2, (0, N * N - 1), (2, 0)) as h:
        assert _call(lib, h, S=1) == -4 and b"crl_tron_sample_mcts_territory: " in lib.crl_last_error() and b"wider than 64" in lib.crl_last_error()
        assert lib.crl_tron_sample_mcts_territory_max_simulations(h, 3) == -4 and b"wider than 64" in lib.crl_last_error()
        assert _call(lib, h, state=(None, D, D, D)) == -1      # (the NULL checks come first, as everywhere)
        assert _call(lib, h, mask=4) == -1 and lib.crl_tron_sample_mcts_territory_max_simulations(h, 4) == -1   # (and the mask's)


@pytest.mark.parametrize("N", SIZES)
def test_s_agent_is_the_restatement(N):
    """S_agent for every mask size: the restatement's number, the header's formula written out once more, m trees of S_agent
    simulations within 64 KB and m trees of one more beyond it (or S_max reached); S_agent passes the check of S, one more
    does not"""
    lib = _lib()
    with tron_context(N, 8, *_layout(N, 8)) as h:
        s_max = lib.crl_tron_mcts_max_simulations(h)
        for m in range(1, 9):
            mask = (1 << m) - 1
            got = lib.crl_tron_sample_mcts_territory_max_simulations(h, mask)
            nwords = -(-N * N // 32)
            assert got == A.agent_max_simulations(N, m) == min(s_max, ((65536 // m) - 8 * nwords) // 16 - 1) and got >= 1
            assert m * T.wave_bytes(N, got) <= 65536 and (got == s_max or m * T.wave_bytes(N, got + 1) > 65536)
            assert lib.crl_tron_sample_mcts_territory_max_simulations(h, mask << (8 - m)) == got     # (the count, not the bits)
            assert _call(lib, h, mask=mask, S=got, flags=2) == -1 and b"flags" in lib.crl_last_error()
            assert _call(lib, h, mask=mask, S=got + 1, flags=2) == -1 and b"S=" in lib.crl_last_error()
    assert A.agent_max_simulations(19, 3) == 1358 and A.agent_max_simulations(64, 8) == 447         # the header's examples


def test_prototypes():
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and _lib().crl_version() == 113
    assert len(_native.PROTOTYPES["crl_tron_sample_mcts_territory"][1]) == 19
    assert len(_native.PROTOTYPES["crl_tron_sample_mcts_territory_max_simulations"][1]) == 2


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TronBatch
    tb = _fake(TronBatch, B=5, P=3, N=7)
    tb.mcts_agent_max_simulations = lambda players=None: 100
    fn = tb.sample_mcts_territory
    for bad in (0, 101, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            fn(bad)
    for bad in (-0.5, 256.0, float("nan"), "1", True, None):
        with pytest.raises(ValueError):
            fn(8, 0, bad)
    for kw in ({"agent": "greedy"}, {"agent": None}, {"noise": -0.5}, {"noise": 1.5}, {"noise": float("nan")}, {"noise": "0.1"},
               {"model_noise": -0.5}, {"model_noise": 1.5}, {"model_noise": float("nan")}, {"model_noise": None},
               {"value_scale": 0}, {"value_scale": 1025}, {"value_scale": 256.0}, {"value_scale": True},
               {"players": [3]}, {"players": [-1]}, {"players": []},
               {"out": torch.zeros((3, 5), dtype=torch.int32)}, {"out": torch.zeros((2, 5), dtype=torch.int8)}):
        with pytest.raises(ValueError):
            fn(8, **kw)
    real = _fake(TronBatch, B=5, P=3, N=7)
    for bad in ([3], [-1], []):
        with pytest.raises(ValueError):
            real.mcts_agent_max_simulations(bad)


def test_vector_env_argument_checks():
    """the new keywords are checked for every opponent, before a device is asked for"""
    from colosseumrl_amd.vector import TronSinglePlayerVectorEnv
    for opponent in TronSinglePlayerVectorEnv.OPPONENTS:
        for kw in ({"simulations": 0}, {"simulations": 4096}, {"simulations": 8.0}, {"simulations": True}, {"exploration": -1.0},
                   {"exploration": 256.0}, {"exploration": "1"}, {"model": "territory"}, {"model": None}, {"model_noise": -0.1},
                   {"model_noise": 1.5}, {"model_noise": "0.1"}):
            with pytest.raises(ValueError):
                TronSinglePlayerVectorEnv(9, 3, 4, opponent=opponent, device="cpu", **kw)
    with pytest.raises(ValueError):
        TronSinglePlayerVectorEnv(9, 3, 4, opponent="mcts", device="cpu")


# ---- the restatement against the two contracts it is made of
def _state(N=7, P=3, B=12, seed=4):
    st = M.positions(N, P, B, np.random.default_rng(seed))
    st.deaths[:, B - 1] = np.arange(P) + 1                       # a finished game: one player alive
    st.deaths[P - 1, B - 1] = 0
    return st


def test_noise_one_is_the_territory_agent_at_noise_one():
    st = _state()
    g = (5 + np.arange(st.B)) & 0xFFFFFFFF
    for players in (None, [1], [0, 2]):
        want = TV.decide(st.N, st.board, st.heads, st.dirs, st.deaths, g, st.tcount, 9, 1.0, players)
        info = A.new_info()
        got = A.sample(st, 6, seed=9, first_env_id=5, noise=1.0, players=players, info=info)
        assert np.array_equal(got, want) and info["searched"] == 0 == info["over"] and info["noisy"] > 0 and info["dead"] > 0
        assert set(np.unique(got)) == {-1, 0, 1}


@pytest.mark.parametrize("agent", ["random", "avoid"])
def test_noise_zero_is_the_search_per_seat(agent):
    st = _state()
    before = [x.copy() for x in (st.board, st.heads, st.dirs, st.deaths, st.tcount)]
    info = A.new_info()
    got = A.sample(st, 10, 100, 128, 9, 5, 0.0, None, agent, 0.2, info=info)
    assert all(np.array_equal(a, b) for a, b in zip(before, (st.board, st.heads, st.dirs, st.deaths, st.tcount)))
    code = np.array([0, 1, -1, 0], np.int8)                      # best 0, 1, 2 and -1 (the last index)
    for p in range(st.P):
        best = T.tron_mcts_territory(st, 10, 100, 128, 9, 5, st.tcount, np.full(st.B, p, np.int8), agent, 0.2)[3]
        assert np.array_equal(got[p], code[best])
        assert ((best == -1) == ((st.deaths[p] != 0) | ((st.deaths == 0).sum(axis=0) < 2))).all()
    assert info["noisy"] == 0 and info["searched"] > 0 and info["dead"] > 0 and info["over"] >= 1
    assert info["searched"] + info["dead"] + info["over"] == st.P * st.B == len(info["picks"]) + info["dead"] + info["over"]


def test_masked_rows_and_mixed_noise():
    st = _state(B=40)
    into = np.full((st.P, st.B), 77, np.int8)
    info = A.new_info()
    got = A.sample(st, 6, seed=3, noise=0.5, players=[0, 2], into=into, info=info)
    assert got is into and (got[1] == 77).all() and (np.abs(got[[0, 2]]) <= 1).all()
    assert info["noisy"] > 5 and info["searched"] > 5
    whole = A.sample(st, 6, seed=3, noise=0.5)
    assert np.array_equal(whole[[0, 2]], got[[0, 2]])            # a player's action does not depend on the mask


def test_gpu_shapes_cover_every_instance():
    """tron_sample_mcts_territory_kernel<P, AVOID, W>: 32.  Reads the list the GPU tests are parametrised with, as
    tests/test_tron_instances_host.py does for the other evaluators."""
    from tests import test_gpu_tron_mcts_agent as G
    from tests import test_gpu_tron_mcts_territory as MT
    name, agents = G.agents.args
    assert name == "agent" and G.SHAPES is MT.SHAPES and len(G.SHAPES) == 20
    got = {(P, a, 32 if N <= 32 else 64) for (N, P), a in itertools.product(G.SHAPES, agents) if N <= 64}
    assert got == set(itertools.product(range(1, 9), ("random", "avoid"), (32, 64))) and len(got) == 32
