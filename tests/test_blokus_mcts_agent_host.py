"""The Blokus search agent (crl_blokus_sample_mcts / crl_blokus_rollout_mcts / crl_blokus_step_single_mcts) on the host: the
argument checks of the three C entries (every CRL_EINVAL case is refused with its message before any device work, the
context's check last), S_max, the prototypes, the counter space of the noise word, the argument checks of the Python wrappers
and the vector env on a batch without a device, and the properties of the plain-Python restatement
(tests/blokus_mcts_agent_ref.py) that need no search."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import blokus_mcts_agent_ref as A
from tests import blokus_mcts_ref as M
from tests import rng_ref as RNG
from tests.host_util import D, fake as _fake, lib as _lib, refused, ttt_context

S_MAX = 1823
NAN = float("nan")
SEARCH = dict(W=8, S=8, Rn=1, cexp=256, noise=0.25)


def _stats(**null):
    from colosseumrl_amd import _native
    names = ("tcount", "tstep", "n_episodes", "win_count", "len_sum", "score_sum", "results")
    return _native.BlokusStats(*[None if null.get(n) else D.value for n in names])


def _sample(lib, ctx=None, B=4, state=(D,) * 6, advance=1, action=D, **kw):
    a = dict(SEARCH, **kw)
    return lib.crl_blokus_sample_mcts(ctx, B, 1, 0, *state, advance, a["W"], a["S"], a["Rn"], a["cexp"], a["noise"], action, None)


def _rollout(lib, ctx=None, B=4, T=3, state=(D,) * 5, stats=None, **kw):
    a = dict(SEARCH, **kw)
    return lib.crl_blokus_rollout_mcts(ctx, B, 1, 0, T, a["W"], a["S"], a["Rn"], a["cexp"], a["noise"], *state,
                                       stats if stats is not None else _stats(), None)


def _single(lib, ctx=None, B=4, state=(D,) * 5, seat=D, learner=D, tcount=D, outs=(D,) * 7, flags=0, **kw):
    a = dict(SEARCH, **kw)
    return lib.crl_blokus_step_single_mcts(ctx, B, 1, 0, *state, seat, learner, tcount, *outs, a["W"], a["S"], a["Rn"], a["cexp"],
                                           a["noise"], flags, None)


ENTRIES = [(_sample, b"crl_blokus_sample_mcts"), (_rollout, b"crl_blokus_rollout_mcts"), (_single, b"crl_blokus_step_single_mcts")]


@pytest.mark.parametrize("call, name", ENTRIES, ids=["sample", "rollout", "step_single"])
def test_search_argument_checks(call, name):
    """what the three entries check alike; no Blokus context can be made without a device, so the context's check, which
    comes last, ends every good call"""
    lib = _lib()
    for B in (0, -1, (1 << 28) + 1):
        refused(lib, call(lib, B=B), name, b"B=")
    for W in (0, 65, -8):
        refused(lib, call(lib, W=W), name, b"W=")
    for S in (0, -1, S_MAX + 1, 65536, 1 << 30):
        refused(lib, call(lib, S=S), name, b"S=")
    for Rn in (0, -3, 1025, 65535):
        refused(lib, call(lib, Rn=Rn), name, b"R=")
    for cexp in (65536, 0xFFFFFFFF):
        refused(lib, call(lib, cexp=cexp), name, b"cexp=")
    for noise in (-0.001, 1.0001, NAN, float("inf"), -float("inf")):
        refused(lib, call(lib, noise=noise), name, b"noise=")
    for good in (dict(), dict(noise=0.0), dict(noise=1.0), dict(W=1, S=1, Rn=1, cexp=0), dict(W=64, S=S_MAX, Rn=1024, cexp=65535)):
        refused(lib, call(lib, **good), name, b"blokus context")
    with ttt_context() as tt:              # a context of another game
        refused(lib, call(lib, ctx=tt), name, b"blokus context")
    # the context's check comes last: a bad argument is named even with a context that would be refused
    refused(lib, call(lib, noise=2.0), b"noise=")
    refused(lib, call(lib, W=0, noise=2.0), b"W=")


def test_max_simulations():
    """S_max stays crl_blokus_mcts's: S_max passes the check of S (a later check stops the call), S_max + 1 does not; the
    word that hands `best` to the other waves fits the spare bytes of a tree's fixed part"""
    lib = _lib()
    assert M.S_MAX == S_MAX
    assert 340 * 2 + 16 + 4 * 64 * 2 == 1208 and 1208 + 4 <= M.FIXED_BYTES
    for call, name in ENTRIES:
        refused(lib, call(lib, S=S_MAX, noise=2.0), name, b"noise=")
        refused(lib, call(lib, S=S_MAX), name, b"blokus context")
        refused(lib, call(lib, S=S_MAX + 1, noise=2.0), name, b"S=")


def test_sample_refuses_what_crl_blokus_sample_refuses():
    lib = _lib()
    for i in range(6):                     # occ, inv, score, round, to_move, tcount
        st = [D] * 6
        st[i] = None
        refused(lib, _sample(lib, state=tuple(st)), b"crl_blokus_sample_mcts", b"NULL pointer")
    refused(lib, _sample(lib, action=None), b"crl_blokus_sample_mcts", b"NULL pointer")
    refused(lib, _sample(lib, action=None, W=0), b"NULL pointer")      # the sibling's checks come first


def test_rollout_refuses_what_crl_blokus_rollout_refuses():
    lib = _lib()
    for i in range(5):
        st = [D] * 5
        st[i] = None
        refused(lib, _rollout(lib, state=tuple(st)), b"crl_blokus_rollout_mcts", b"NULL state")
    for n in ("tcount", "tstep", "n_episodes", "win_count", "len_sum", "score_sum"):
        refused(lib, _rollout(lib, stats=_stats(**{n: True})), b"crl_blokus_rollout_mcts", b"NULL stats")
    refused(lib, _rollout(lib, stats=_stats(results=True)), b"blokus context")         # results may be NULL
    for T in (-1, (1 << 24) + 1):
        refused(lib, _rollout(lib, T=T), b"crl_blokus_rollout_mcts", b"T=")
    refused(lib, _rollout(lib, T=0), b"blokus context")                                 # T = 0 is checked like any other
    refused(lib, _rollout(lib, T=0, S=0), b"S=")
    refused(lib, _rollout(lib, T=1 << 24), b"blokus context")


def test_step_single_refuses_what_crl_blokus_step_single_refuses():
    lib = _lib()
    name = b"crl_blokus_step_single_mcts"
    for i in range(5):
        st = [D] * 5
        st[i] = None
        refused(lib, _single(lib, state=tuple(st)), name, b"NULL state")
    refused(lib, _single(lib, seat=None), name, b"seat")
    refused(lib, _single(lib, tcount=None), name, b"tcount")
    for i in range(7):
        outs = [D] * 7
        outs[i] = None
        refused(lib, _single(lib, outs=tuple(outs)), name, b"NULL output")
    for flags in (1, 4, 0x80000000):       # CRL_STEP_RANK_ACTION is the one it knows
        refused(lib, _single(lib, flags=flags), name, b"flags")
    from colosseumrl_amd._native import CRL_STEP_RANK_ACTION
    refused(lib, _single(lib, flags=CRL_STEP_RANK_ACTION), name, b"blokus context")
    outs = [D] * 7
    outs[4] = C.c_void_p(66)               # obs_board
    refused(lib, _single(lib, outs=tuple(outs)), name, b"aligned")
    refused(lib, _single(lib, learner=None), name, b"blokus context")                   # no learner ply: allowed


def test_prototypes_abi_and_tags():
    import os
    import re
    from colosseumrl_amd import _native
    lib = _lib()
    assert _native.CRL_ABI_VERSION == 113 and lib.crl_version() == 113
    for name, n_args in (("crl_blokus_sample_mcts", 18), ("crl_blokus_rollout_mcts", 17), ("crl_blokus_step_single_mcts", 26)):
        assert name in _native.PROTOTYPES and len(_native.PROTOTYPES[name][1]) == n_args
        assert getattr(lib, name).argtypes is not None and C.c_double in _native.PROTOTYPES[name][1]
    assert "crl_blokus_rollout_mcts_bind" not in _native.PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = open(os.path.join(root, "colosseumrl_amd", "csrc", "crl_common.hpp")).read()
    assert len(re.findall(r"#define\s+CRL_TAG_\w+", common)) == 12       # the agent has no tag of its own
    header = open(os.path.join(root, "include", "colosseum_hip.h")).read()
    assert all(("int %s(" % n) in header for n in ("crl_blokus_sample_mcts", "crl_blokus_rollout_mcts", "crl_blokus_step_single_mcts"))


def test_noise_word_has_a_counter_space_of_its_own():
    """the noise word's second counter word has both top bits set: the playouts' have bit 30 alone, the widening draws' bit
    31 alone, crl_blokus_playout's neither -- so for the same (g, c) the blocks, hence the words, differ"""
    from tests.blokus_ref import blokus_word
    rng = np.random.default_rng(23)
    assert A.NOISE_BITS == M.PLAYOUT_BIT | M.WIDEN_BIT
    for _ in range(50):
        seed, g, c = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))
        u = A.noise_word(seed, g, c)
        assert u != M.playout_word(seed, g, c, 0, 0)
        assert u != int(RNG.philox(g, M.WIDEN_BIT | (c >> 2), 0, M.TAG, seed)[c & 3])
        assert u != M.widen_word(seed, g, c >> 2, 0) or (c & 3) != 0
        assert u != blokus_word(seed, g, c, 0, RNG.CRL_TAG_BLOKUS_PLAYOUT)
        assert u != blokus_word(seed, g, c)                                        # the random agent's word: another tag
        assert u == int(RNG.philox(g, 0xC0000000 | (c >> 2), 0, 0x42500000, seed)[c & 3])
    for c in (0, 5, 2 ** 32 - 1):
        second = A.NOISE_BITS | (c >> 2)
        assert second >= 0xC0000000 > (M.WIDEN_BIT | 336) and second < 2 ** 32
        assert ((c >> 2) | M.PLAYOUT_BIT) < 0x80000000 <= (M.WIDEN_BIT | 0)


def test_threshold():
    assert A.threshold(0.0) == 0 and A.threshold(1.0) == 2 ** 32 and A.threshold(0.5) == 2 ** 31
    assert A.threshold(2.0 ** -32) == 1 and A.threshold(2.0 ** -33) == 1 and A.threshold(1.0 - 2.0 ** -33) == 2 ** 32
    assert all(not (u < A.threshold(0.0)) and u < A.threshold(1.0) for u in (0, 1, 2 ** 32 - 1))     # never / always noisy
    assert A.threshold(0.3) == math.ceil(0.3 * 2 ** 32) == RNG.threshold(0.3)


# ---- the restatement's rules that need no search
@pytest.fixture(scope="module")
def positions():
    """a fresh game, a round-6 board with small inventories whose mover has a choice, a late game whose mover must pass
    while another player can move, and a finished game"""
    from oracle import oracle as O
    from tests import blokus_positions as BP
    tiny, late = BP.tiny_inventories(12), BP.late(24)
    n_legal = BP.counts(tiny)[np.arange(tiny.B), tiny.to_move & 3]
    a = int(np.flatnonzero(n_legal >= 6)[0])
    b = int(np.flatnonzero(BP.late_kinds(late)[0] >= 1)[0])
    st = BP.concat([O.BlokusState(1), BP.clone(tiny, [a]), BP.clone(late, [b]), BP.finished(1)])
    st.tcount[:] = [0, 7, 2 ** 32 - 1, 30]
    return st


def test_noise_one_is_the_random_agent(positions, monkeypatch):
    from tests.blokus_ref import blokus_draw_rank, blokus_list, blokus_one
    monkeypatch.setattr(M, "search", lambda *a, **k: pytest.fail("a noisy ply searched"))
    st = positions
    log = []
    before = st.tcount.copy()
    act = A.sample_mcts(st, 91, 8, 16, 1, 256, 1.0, first_env_id=2 ** 32 - 2, advance=True, log=log)
    assert (st.tcount == before + np.uint32(1)).all()                               # passes included, and it wraps
    st.tcount[:] = before
    for b in range(st.B):
        ids = blokus_list(blokus_one(st, b))
        g = (2 ** 32 - 2 + b) & 0xFFFFFFFF
        want = int(ids[blokus_draw_rank(91, g, int(before[b]), len(ids))]) if len(ids) else -1
        assert act[b] == want
    assert [k for _, _, k in log] == ["noisy", "noisy", "pass", "pass"]
    again = A.sample_mcts(st, 91, 8, 16, 1, 256, 1.0, first_env_id=2 ** 32 - 2, advance=False)
    assert (again == act).all() and (st.tcount == before).all()


def test_no_actions_is_a_pass_without_a_search(positions, monkeypatch):
    from tests.blokus_ref import blokus_one
    monkeypatch.setattr(M, "search", lambda *a, **k: pytest.fail("a mover without actions searched"))
    monkeypatch.setattr(A, "noise_word", lambda *a: pytest.fail("a mover without actions drew"))
    for b in (2, 3):
        for noise in (0.0, 0.5, 1.0):
            kinds = []
            assert A.agent_action(blokus_one(positions, b), 5, 9, 1, 8, 16, 1, 256, noise, kinds) == -1 and kinds == ["pass"]


def test_noise_zero_is_the_search(positions, monkeypatch):
    from tests.blokus_ref import blokus_one
    seen = []

    def search(one, S, R, W, cexp, seed, g, tc):
        seen.append((S, R, W, cexp, seed, g, tc))
        return [], [], [], 0, 4242
    monkeypatch.setattr(M, "search", search)
    kinds = []
    assert A.agent_action(blokus_one(positions, 1), 7, 12, 3, 5, 16, 2, 128, 0.0, kinds) == 4242 and kinds == ["searched"]
    assert seen == [(16, 2, 5, 128, 3, 12, 7)]                                     # the ply's counter is the search's tcount


# ---- the Python wrappers refuse bad arguments before they reach the library (no device needed to get there)
def _fake_batch():
    from colosseumrl_amd.batched import BlokusBatch
    bb = _fake(BlokusBatch, B=3, P=4)
    bb.__dict__["mcts_max_simulations"] = S_MAX
    return bb


def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    assert BlokusBatch.OPPONENTS == ("random", "mcts")
    bb = _fake_batch()
    for fn in (bb.sample_mcts, lambda *a, **k: bb.rollout_mcts(4, *a, **k)):
        for bad in (0, S_MAX + 1, -1, 2.0, True, None):
            with pytest.raises(ValueError):
                fn(bad)
        for bad in (0, 1025, 16.0, False):
            with pytest.raises(ValueError):
                fn(8, bad)
        for bad in (0, 65, 8.0, True):
            with pytest.raises(ValueError):
                fn(8, 1, bad)
        for bad in (-0.5, 256.0, NAN, "1", True, None):
            with pytest.raises(ValueError):
                fn(8, 1, 8, 0, bad)
        for bad in (-0.1, 1.5, NAN, "0", True, None):
            with pytest.raises(ValueError):
                fn(8, 1, 8, 0, 1.0, bad)
    seat = torch.zeros(3, dtype=torch.int8)
    for kw in (dict(opponent="tactical"), dict(opponent=None), dict(noise=-0.1), dict(noise=NAN), dict(simulations=0),
               dict(simulations=S_MAX + 1), dict(playouts=0), dict(playouts=1025), dict(width=0), dict(width=65),
               dict(exploration=-1.0), dict(exploration=NAN)):
        for opponent in ("random", "mcts"):    # every keyword is checked whoever the opponent is
            with pytest.raises(ValueError):
                bb.step_single(seat, None, **dict(dict(opponent=opponent), **kw))
    with pytest.raises(ValueError):
        bb.step_single(torch.zeros(3, dtype=torch.int32), opponent="mcts")


def test_env_argument_checks(monkeypatch):
    from colosseumrl_amd import vector
    from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv
    made = []

    class Batch:
        device = "cpu"

        def __init__(self, batch, device=None):
            made.append(batch)
    monkeypatch.setattr(vector, "BlokusBatch", type("B", (Batch,), {"OPPONENTS": ("random", "mcts")}))
    monkeypatch.setattr(vector, "_seat_tensor", lambda *a: None)
    for kw in (dict(opponent="avoid"), dict(noise=1.5), dict(noise=NAN), dict(simulations=0), dict(simulations=S_MAX + 1),
               dict(simulations=8.0), dict(playouts=0), dict(playouts=1025), dict(width=0), dict(width=65), dict(exploration=-1),
               dict(exploration=256.0)):
        for opponent in ("random", "mcts"):
            with pytest.raises(ValueError):
                BlokusSinglePlayerVectorEnv(8, **dict(dict(opponent=opponent), **kw))
    assert not made                                                 # refused before a batch is made
    env = BlokusSinglePlayerVectorEnv(8, opponent="mcts", noise=0.25, simulations=S_MAX, playouts=5, width=3, exploration=0.5)
    assert made == [8] and env.opponent == "mcts"
    assert env._search == dict(noise=0.25, simulations=S_MAX, playouts=5, width=3, exploration=0.5)
    assert BlokusSinglePlayerVectorEnv(8).opponent == "random"
