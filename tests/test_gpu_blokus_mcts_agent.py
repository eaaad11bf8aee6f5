"""The Blokus search agent (crl_blokus_sample_mcts / crl_blokus_rollout_mcts / crl_blokus_step_single_mcts) on the GPU:
bit-exact against the plain-Python restatement (tests/blokus_mcts_agent_ref.py) with both mappings (R = 1: a wave per game,
R = 5: a workgroup per game), against crl_blokus_mcts and the random agent's entries on the GPU itself, the vector env eagerly
and from a captured graph, and the agent's strength as an opponent.

The restatement costs 0.2-0.3 s per search from the empty board at S = 8, R = 1 and about 1.2 s at S = 6, R = 5, so the
bit-exact cases use S = 8 (R = 1) and S = 6 (R = 5) with W = 3 -- the root has its three children after six simulations, the
later ones select and expand at depth 2 -- on at most 8 games, and every GPU and CPU result is computed once."""
import functools

import numpy as np
import pytest

from tests import blokus_mcts_agent_ref as A
from tests import blokus_positions as BP
from tests.blokus_ref import blokus_list, blokus_one
from tests.gpu_util import DEV, blokus_batch, first_episodes, np_of, u32_of

pytestmark = pytest.mark.gpu

SEED, FIRST_ENV_ID, W = 0x5EA7C4, 4000, 3
S_OF = {1: 8, 5: 6}                        # simulations by playouts per leaf
STATE = ("occ", "inv", "score", "round", "to_move")
NAMES = ["empty", "plies12", "plies40", "must_pass", "finished", "tcount_wrap", "tiny2"]


def _search(Rn, noise=0.0):
    return (W, S_OF[Rn], Rn, 256, noise)


def _kw(Rn, noise=0.0):
    return dict(simulations=S_OF[Rn], playouts=Rn, width=W, exploration=1.0, noise=noise)


def _state_of(bb):
    return {k: u32_of(getattr(bb, k)).copy() for k in STATE + ("tcount",)}


def _same_state(bb, st, tcount=None):
    for k in STATE:
        assert np.array_equal(u32_of(getattr(bb, k)), getattr(st, k).view(np.uint32)), k
    assert np.array_equal(u32_of(bb.tcount), st.tcount if tcount is None else tcount)


def _mid_games(B, plies, seed=77, first=9100):
    from oracle import oracle as O
    st = O.BlokusState(B)
    O.blokus_rollout(st, seed, first, plies, n_threads=BP.THREADS)
    assert not st.n_episodes.any()
    return BP.clone(st)


# ------------------------------------------------------------------ sample_mcts
@functools.lru_cache(maxsize=None)
def _positions():
    """(state of seven positions, tcount): test_gpu_blokus_mcts's six -- the empty board; a game after 12 and one after 40
    random plies; one whose mover must pass while another player can move; a finished game; a small position at tcount =
    2^32 - 2 -- and a second small position, so that the last workgroup of the wave-per-game mapping has an idle wave"""
    from oracle import oracle as O
    empty, p12, p40 = O.BlokusState(1), O.BlokusState(1), O.BlokusState(1)
    O.blokus_rollout(p12, 41, 500, 12)
    O.blokus_rollout(p40, 42, 501, 40)
    assert not p12.n_episodes.any() and not p40.n_episodes.any()
    late = BP.late(24)
    must_pass = BP.clone(late, [int(np.flatnonzero(BP.late_kinds(late)[0] >= 1)[0])])
    tiny = BP.tiny_inventories(12)
    n_legal = BP.counts(tiny)[np.arange(tiny.B), tiny.to_move & 3]
    roomy = np.flatnonzero(n_legal >= 6)
    st = BP.concat([empty, p12, p40, must_pass, BP.finished(1), BP.clone(tiny, [int(roomy[0])]), BP.clone(tiny, [int(roomy[1])])])
    legal = [len(blokus_list(blokus_one(st, b))) for b in range(st.B)]
    assert min(legal[:3]) > 0 and legal[3] == 0 and legal[4] == 0 and min(legal[5:]) >= 6
    assert BP.counts(st)[3].sum() > 0 and BP.counts(st)[4].sum() == 0
    return st, np.array([0, 5, 13, 9, 3, 2 ** 32 - 2, 21], np.uint32)


@functools.lru_cache(maxsize=None)
def _gpu_sample(Rn):
    """(actions of sample_mcts(noise = 0, advance = False), `best` of mcts on the same positions)"""
    st, tcount = _positions()
    bb = blokus_batch(st, FIRST_ENV_ID, tcount)
    act = np_of(bb.sample_mcts(seed=SEED, advance=False, **_kw(Rn))).copy()
    best = np_of(bb.mcts(S_OF[Rn], Rn, None, W, SEED, 1.0)["best"]).copy()
    return act, best


@pytest.mark.parametrize("Rn", [1, 5])
@pytest.mark.parametrize("b", range(7), ids=NAMES)
def test_sample_bit_exact(b, Rn):
    st, tcount = _positions()
    act, best = _gpu_sample(Rn)
    kinds = []
    want = A.agent_action(blokus_one(st, b), int(tcount[b]), FIRST_ENV_ID + b, SEED, *_search(Rn), kinds=kinds)
    print(act[b], best[b], want, kinds)
    assert act[b] == want and act[b] == best[b]
    if b in (3, 4):
        assert want == -1 and kinds == ["pass"]                 # the must-pass and the finished row
    else:
        assert want >= 0 and kinds == ["searched"]


def test_sample_advance_repeatable_and_read_only():
    st, tcount = _positions()
    for Rn in (1, 5):
        bb = blokus_batch(st, FIRST_ENV_ID, tcount)
        before = _state_of(bb)
        first = np_of(bb.sample_mcts(seed=SEED, advance=False, **_kw(Rn))).copy()
        again = np_of(bb.sample_mcts(seed=SEED, advance=False, **_kw(Rn))).copy()
        assert np.array_equal(first, again) and np.array_equal(first, _gpu_sample(Rn)[0])
        after = _state_of(bb)
        assert all(np.array_equal(before[k], after[k]) for k in before)             # without advance nothing is written
        moved = np_of(bb.sample_mcts(seed=SEED, advance=True, **_kw(Rn))).copy()
        after = _state_of(bb)
        assert np.array_equal(moved, first)
        assert np.array_equal(after["tcount"], tcount + np.uint32(1))               # every row, the passes and the wrap included
        assert all(np.array_equal(before[k], after[k]) for k in STATE)


def test_sample_placement_independence():
    """a position gives the same action wherever it sits in the batch, when first_env_id is shifted to keep its game id"""
    st, tcount = _positions()
    pad = 3
    wide = BP.concat([BP.clone(st, [2] * pad), st])
    bb = blokus_batch(wide, FIRST_ENV_ID - pad, np.concatenate([np.full(pad, 77, np.uint32), tcount]))
    for Rn in (1, 5):
        act = np_of(bb.sample_mcts(seed=SEED, advance=False, **_kw(Rn)))
        assert np.array_equal(act[pad:], _gpu_sample(Rn)[0])


# ------------------------------------------------------------------ noise
@pytest.mark.parametrize("Rn", [1, 5])
def test_noise_one_is_the_random_agent(Rn):
    """at noise 1 every ply is noisy: sample_mcts is sample, and the step against the search is the step against the random
    agent -- state, counters and outputs"""
    import torch
    st, tcount = _positions()
    mid = _mid_games(25, 30)
    both = BP.concat([st, mid])
    tc = np.concatenate([tcount, BP.counters(mid.B)])
    a, b = blokus_batch(both, FIRST_ENV_ID, tc), blokus_batch(both, FIRST_ENV_ID, tc)
    assert torch.equal(a.sample_mcts(seed=SEED, **_kw(Rn, 1.0)), b.sample(SEED))
    assert torch.equal(a.tcount, b.tcount)
    seat = torch.from_numpy((np.arange(both.B) % 4).astype(np.int8)).to(DEV)
    rng = np.random.default_rng(5)
    for t in range(4):
        act = None if t == 0 else torch.from_numpy(rng.integers(-1, 60, size=both.B)).to(DEV)
        oa = a.step_single(seat, act, SEED, rank=True, opponent="mcts", **_kw(Rn, 1.0))
        ob = b.step_single(seat, act, SEED, rank=True)
        assert oa.keys() == ob.keys()
        for k in oa:
            assert torch.equal(oa[k], ob[k]), k
        for k in STATE + ("tcount",):
            assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("Rn", [1, 5])
def test_rollout_noise_one_is_the_rollout(Rn):
    """64 games, 12 plies: rollout_mcts(noise = 1) leaves the state, the counters and the results rows of rollout"""
    import torch
    late, mid = BP.late(24), _mid_games(40, 44)
    st = BP.concat([late, mid])
    tc = BP.counters(st.B)
    a, b = blokus_batch(st, 31, tc), blokus_batch(st, 31, tc)
    a.rollout_mcts(12, seed=SEED, **_kw(Rn, 1.0))
    b.rollout(12, SEED)
    for k in STATE + ("tcount", "tstep", "n_episodes", "len_sum", "win_count", "score_sum"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.results(), b.results()) and int(a.n_episodes.sum()) >= 8


@functools.lru_cache(maxsize=None)
def _half_noise():
    """(state of twelve positions, tcount, seed): the seven positions and five games after 20 .. 52 plies; the seed is the
    first under which at least 4 of the ten movers with actions draw a noisy ply and at least 4 search"""
    st, tcount = _positions()
    more = [_mid_games(1, plies, 300 + plies, 60 + plies) for plies in (20, 28, 36, 44, 52)]
    both = BP.concat([st] + more)
    tc = np.concatenate([tcount, np.array([20, 28, 36, 44, 52], np.uint32)])
    can = [b for b in range(both.B) if len(blokus_list(blokus_one(both, b)))]
    assert len(can) == 10
    thr = A.threshold(0.5)
    for seed in range(1000, 1100):
        noisy = sum(A.noise_word(seed, FIRST_ENV_ID + b, int(tc[b])) < thr for b in can)
        if 4 <= noisy <= len(can) - 4:
            return both, tc, seed
    raise AssertionError("no seed with 4 noisy and 4 searched plies")


@pytest.mark.parametrize("Rn", [1, 5])
def test_noise_half_bit_exact(Rn):
    st, tc, seed = _half_noise()
    bb = blokus_batch(st, FIRST_ENV_ID, tc)
    act = np_of(bb.sample_mcts(seed=seed, **_kw(Rn, 0.5)))
    ref, log = BP.clone(st), []
    ref.tcount[:] = tc
    want = A.sample_mcts(ref, seed, *_search(Rn, 0.5), first_env_id=FIRST_ENV_ID, log=log)
    kinds = [k for _, _, k in log]
    print(act.tolist(), want.tolist(), kinds)
    assert kinds.count("noisy") >= 4 and kinds.count("searched") >= 4 and kinds.count("pass") == 2
    assert np.array_equal(act, want) and np.array_equal(u32_of(bb.tcount), ref.tcount)


# ------------------------------------------------------------------ step_single against the restatement
@functools.lru_cache(maxsize=None)
def _single_positions():
    """(state of eight games, tcount, seat): the empty board, games after 12 and 40 plies, rows 0, 1, 3, 4 of
    blokus_positions.late(12) -- 1 and 4 end on the next ply, in 0 and 3 two movers in a row must pass -- and one of
    tiny_inventories.  The seats: in games 1, 5 and 6 it is the learner's turn at entry; in game 3 two opponents pass before
    one searches; in game 4 the opponent's ply ends the game and two opponents open the next one from the empty board."""
    from oracle import oracle as O
    empty, p12, p40 = O.BlokusState(1), O.BlokusState(1), O.BlokusState(1)
    O.blokus_rollout(p12, 41, 500, 12)
    O.blokus_rollout(p40, 42, 501, 40)
    late = BP.late(12)
    passes, ends = BP.late_kinds(late)
    assert passes[[0, 3]].tolist() == [2, 2] and ends[[1, 4]].all()
    assert BP.counts(late)[[1, 4], late.to_move[[1, 4]] & 3].tolist() == [2, 2]
    st = BP.concat([empty, p12, p40, BP.clone(late, [0, 1, 3, 4]), BP.clone(BP.tiny_inventories(12), [0])])
    seat = np.array([1, 0, 2, 1, 2, 2, 3, 3], np.int8)
    assert ((st.to_move & 3) == seat).tolist() == [False, True, False, False, False, True, True, False]
    return st, np.array([0, 12, 40, 7, 2 ** 32 - 2, 15, 16, 3], np.uint32), seat


SINGLE_KEYS = ("reward", "done", "winners", "n_valid", "board", "pieces", "score")
# the second call's ranks: the first action, later ones, one outside the list (a pass), the second of the two actions that
# end game 6
RANKS = np.array([0, 5, 17, 1, 3, 0, 1, 10 ** 6], np.int64)


@functools.lru_cache(maxsize=None)
def _cpu_single(Rn):
    """the restatement's two calls: learner_action = None, then RANKS by rank -> (outputs, state, tcount) per call, the log"""
    st0, tcount, seat = _single_positions()
    st, log, calls = BP.clone(st0), [], []
    st.tcount[:] = tcount
    for act in (None, RANKS):
        log.append("call")
        out = A.step_single_mcts(st, seat, act, SEED, *_search(Rn), first_env_id=FIRST_ENV_ID, rank=True, log=log)
        calls.append((out, BP.clone(st), st.tcount.copy()))
    return calls, log


@functools.lru_cache(maxsize=None)
def _gpu_single(Rn):
    import torch
    st0, tcount, seat = _single_positions()
    bb = blokus_batch(st0, FIRST_ENV_ID, tcount)
    seat_t, calls = torch.from_numpy(seat).to(DEV), []
    for act in (None, RANKS):
        o = bb.step_single(seat_t, None if act is None else torch.from_numpy(act).to(DEV), SEED, rank=True, opponent="mcts",
                           **_kw(Rn))
        calls.append(({k: np_of(o[k]).copy() for k in SINGLE_KEYS}, _state_of(bb)))
    return calls


def test_step_single_cases_are_what_they_claim():
    """from the restatement's log, so that the comparison below cannot go soft: searched plies in a row inside one call (the
    board put back after a search, the counter advancing), an opponent who passes without a search, a game that ends and
    restarts inside a call with a search from the empty board behind it"""
    _, log = _cpu_single(1)
    runs, passes, reopened = {}, 0, 0
    call, streak, restarted = 0, {}, set()
    for e in log:
        if e == "call":
            call, streak, restarted = call + 1, {}, set()
            continue
        b, c, kind = e
        if kind == "searched":
            streak[b] = streak.get(b, 0) + 1
            runs[(call, b)] = max(runs.get((call, b), 0), streak[b])
            reopened += b in restarted
        else:
            streak[b] = 0
        passes += kind == "pass"
        if kind == "restart":
            restarted.add(b)
    assert len(set(b for (_, b), n in runs.items() if n >= 2)) >= 2
    assert passes >= 1 and reopened >= 1
    assert sum(1 for e in log if e != "call" and e[2] == "learner") == 8              # the second call: every learner plays


@pytest.mark.parametrize("call", [0, 1], ids=["advance_to_the_learner", "ranks"])
@pytest.mark.parametrize("Rn", [1, 5])
def test_step_single_bit_exact(Rn, call):
    (want, st, tc), (got, state) = _cpu_single(Rn)[0][call], _gpu_single(Rn)[call]
    for k in STATE:
        assert np.array_equal(state[k], getattr(st, k).view(np.uint32)), k
    assert np.array_equal(state["tcount"], tc)
    for k, w in zip(SINGLE_KEYS, want):
        assert np.array_equal(got[k], w), k
    if call == 1:
        assert got["done"].sum() >= 1


@pytest.mark.parametrize("Rn", [1, 5])
def test_step_single_ids_and_error_codes(Rn):
    """learner actions by id: one per CRL_BLOKUS_*_ERROR code -- the game and its counter stay as they were and no opponent
    plays -- beside a pass, after which the opponents pass or search"""
    import torch
    from oracle import oracle as O
    p12 = O.BlokusState(1)
    O.blokus_rollout(p12, 41, 500, 12)
    late = BP.late(12)
    st = BP.concat([p12, p12, p12, BP.clone(late, [3])])
    seat = np.array([0, 0, 0, 2], np.int8)
    assert ((st.to_move & 3) == seat).all()
    gone = next(p for p in range(21) if not (int(st.inv[0, 0]) >> p) & 1)
    act = np.array([O.blokus_encode(gone, 10, 10, 0, 0),       # a piece the learner no longer holds: CRL_BLOKUS_VALUE_ERROR
                    O.blokus_encode(0, 10, 10, 0, 1),          # a shift that names no cell of the monomino: CRL_BLOKUS_INDEX_ERROR
                    336000 + 1344000 + 5,                      # no action id at all: CRL_BLOKUS_BAD_ACTION
                    -1], np.int64)
    tcount = np.array([12, 12, 12, 9], np.uint32)
    bb = blokus_batch(st, FIRST_ENV_ID, tcount)
    o = bb.step_single(torch.from_numpy(seat).to(DEV), torch.from_numpy(act).to(DEV), SEED, opponent="mcts", **_kw(Rn))
    ref, log = BP.clone(st), []
    ref.tcount[:] = tcount
    want = A.step_single_mcts(ref, seat, act, SEED, *_search(Rn), first_env_id=FIRST_ENV_ID, log=log)
    assert want[0].tolist()[:3] == [-2, -1, -3] and want[0][3] == 0
    assert [e for e in log if e[0] < 3] == [(0, 12, "learner"), (1, 12, "learner"), (2, 12, "learner")]   # no opponent played
    assert sum(1 for e in log if e[0] == 3 and e[2] == "searched") >= 1
    _same_state(bb, ref)
    for k in STATE:                                             # the three games are what they were
        assert np.array_equal(u32_of(getattr(bb, k))[:3], getattr(st, k).view(np.uint32)[:3]), k
    assert np.array_equal(u32_of(bb.tcount)[:3], tcount[:3])
    for k, w in zip(SINGLE_KEYS, want):
        assert np.array_equal(np_of(o[k]), w), k


# ------------------------------------------------------------------ rollout_mcts
@functools.lru_cache(maxsize=None)
def _rollout_positions():
    late = BP.late(12)
    st = BP.concat([BP.clone(late, [0, 1, 2, 4, 5, 7]), _mid_games(1, 24, 301, 70), _mid_games(1, 44, 302, 71)])
    return st, np.array([3, 2 ** 32 - 3, 14, 15, 16, 0, 24, 44], np.uint32)


@pytest.mark.parametrize("Rn", [1, 5])
def test_rollout_is_sample_then_step(Rn):
    """T x (sample_mcts; step with auto-reset) == rollout_mcts(T): state, counters and results rows (the composition's rows
    are counted here: the final scores come from a twin that plays the ply without the reset); two games also against the
    restatement"""
    import torch
    T = 4
    st, tcount = _rollout_positions()
    a, b, probe = blokus_batch(st, 31, tcount), blokus_batch(st, 31, tcount), blokus_batch(st, 31, tcount)
    a.rollout_mcts(T, seed=SEED, **_kw(Rn))
    rows, ts = np.zeros((st.B, 10), np.int64), np.zeros(st.B, np.int64)
    for _ in range(T):
        act = b.sample_mcts(seed=SEED, **_kw(Rn))
        for k in STATE:
            getattr(probe, k).copy_(getattr(b, k))
        probe.step(act, auto_reset=False)
        final = np_of(probe.score).astype(np.int64)
        _, term, ws = b.step(act, auto_reset=True)
        term, ws = np_of(term).astype(bool), np_of(ws).astype(np.int64)
        ts += 1
        rows[term, 0] += 1
        rows[term, 1] += ts[term]
        for q in range(4):
            rows[term, 2 + q] += (ws[term] >> q) & 1
            rows[term, 6 + q] += final[term, q]
        ts[term] = 0
    for k in STATE + ("tcount",):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(np_of(a.results()).astype(np.int64), rows) and np.array_equal(np_of(a.tstep).astype(np.int64), ts)
    assert np.array_equal(np_of(a.results_from_columns()), np_of(a.results())) and rows[:, 0].sum() >= 2
    games = [1, 6]                                             # one that ends on its first ply, one in mid game
    ref, log = BP.clone(st), []
    ref.tcount[:] = tcount
    A.rollout_mcts(ref, T, SEED, *_search(Rn), first_env_id=31, log=log, games=games)
    assert sum(1 for e in log if e[2] == "searched") >= 6
    for k in STATE:
        assert np.array_equal(u32_of(getattr(a, k))[games], getattr(ref, k).view(np.uint32)[games]), k
    for k in ("tcount", "tstep", "n_episodes", "len_sum"):
        assert np.array_equal(u32_of(getattr(a, k))[games], getattr(ref, k)[games]), k
    for k in ("win_count", "score_sum"):
        assert np.array_equal(u32_of(getattr(a, k))[:, games], getattr(ref, k).view(np.uint32)[:, games]), k
    assert ref.n_episodes[1] == 1


def test_rollout_zero_steps():
    st, tcount = _rollout_positions()
    bb = blokus_batch(st, 31, tcount)
    before = _state_of(bb)
    bb.rollout_mcts(0, seed=SEED, **_kw(1))
    after = _state_of(bb)
    assert all(np.array_equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------ the vector env
def test_vector_env_graph_replay():
    """opponent="mcts" stepped eagerly equals the same steps replayed from a captured graph (a single kernel: no parallel
    branches); the pattern of test_blokus_vector_env_graph_replay"""
    import torch
    from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv
    B = 37

    def make():
        seat = torch.from_numpy((np.arange(B) % 4).astype(np.int8))
        return BlokusSinglePlayerVectorEnv(B, seat=seat, seed=9, action="rank", device=DEV, opponent="mcts", noise=0.25,
                                           simulations=8, playouts=1, width=3)
    eager, graphed = make(), make()
    eager.reset(), graphed.reset()
    action = torch.zeros((B,), dtype=torch.int64, device=DEV)
    rng = np.random.default_rng(11)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    a = torch.from_numpy(rng.integers(-1, 400, size=B)).to(DEV)
    action.copy_(a)
    with torch.cuda.stream(s):
        graphed.step(action)                                        # warm-up on a side stream, as torch.cuda.graph wants
    torch.cuda.current_stream().wait_stream(s)
    eager.step(a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = graphed.step(action)
    n_done = 0
    for _ in range(30):
        a = torch.from_numpy(rng.integers(-1, 400, size=B)).to(DEV)
        action.copy_(a)
        want = eager.step(a)
        want = [{k: v.clone() for k, v in w.items()} if isinstance(w, dict) else w.clone() for w in want]
        g.replay()
        torch.cuda.synchronize()
        for w, r in zip(want, res):
            if isinstance(w, dict):
                assert w.keys() == r.keys()
                for k in w:
                    assert torch.equal(w[k], r[k]), k
            else:
                assert torch.equal(w, r)
        n_done += int(want[2].sum())
    for k in STATE + ("tcount",):
        assert torch.equal(getattr(eager.batch, k), getattr(graphed.batch, k)), k
    assert n_done > 0


def test_vector_env_random_opponent_is_unchanged():
    """opponent="random" -- the default, whatever the search keywords say -- steps as step_single against the random agent"""
    import torch
    from colosseumrl_amd.batched import BlokusBatch
    from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv
    B = 16
    env = BlokusSinglePlayerVectorEnv(B, seat=1, seed=9, action="rank", device=DEV, noise=0.5, simulations=5, playouts=7, width=2)
    plain = BlokusSinglePlayerVectorEnv(B, seat=1, seed=9, action="rank", device=DEV)
    twin = BlokusBatch(B, device=DEV)
    seat = torch.full((B,), 1, dtype=torch.int8, device=DEV)
    assert env.opponent == "random" and plain.opponent == "random"
    env.reset(), plain.reset()
    o = twin.step_single(seat, None, 9, rank=True)
    rng = np.random.default_rng(3)
    for _ in range(6):
        a = torch.from_numpy(rng.integers(0, 50, size=B)).to(DEV)
        obs, reward, done, info = env.step(a)
        obs2, reward2, done2, info2 = plain.step(a)
        o = twin.step_single(seat, a, 9, rank=True, out=o)
        assert torch.equal(obs["board"], o["board"]) and torch.equal(reward, o["reward"]) and torch.equal(done, o["done"])
        assert torch.equal(info["n_valid"], o["n_valid"]) and torch.equal(obs2["board"], o["board"])
        assert torch.equal(reward2, o["reward"]) and torch.equal(info2["n_valid"], o["n_valid"])
        for k in STATE + ("tcount",):
            assert torch.equal(getattr(env.batch, k), getattr(twin, k)), k


# ------------------------------------------------------------------ strength
STRENGTH_GAMES = 128
STRENGTH_MARGIN = 0.527                    # half the gap measured on an MI355X (see the docstring below)


def _mean_final_rank(opponent):
    import torch
    from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv
    env = BlokusSinglePlayerVectorEnv(STRENGTH_GAMES, seat=0, seed=2024, action="rank", device=DEV, opponent=opponent, noise=0.0,
                                      simulations=32, playouts=1, width=8)
    env.reset()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)

    def policy(env, t):
        n = env._out["n_valid"].to(torch.float64)
        u = torch.rand(STRENGTH_GAMES, generator=gen, device=DEV, dtype=torch.float64)
        return torch.minimum((u * n).to(torch.int64), (n - 1).clamp(min=0).to(torch.int64))
    last, _, _ = first_episodes(env, policy, 60)
    return float(last.to(torch.float64).mean())


def test_strength_as_an_opponent():
    """A uniformly random learner (by rank, seat 0, the first episode of each of 128 games) finishes lower against three
    searches (S = 32, R = 1, W = 8, noise 0) than against three random agents.  The reward at the end of a game is the
    learner's rank in the final scores, 0 = last .. 3 = best.
    Measured on an MI355X when the agent was built: 1.7812 against random agents, 0.7266 against the searches, a gap of
    1.0547; the margin is half that gap, 0.527.  With 128 games each mean resolves to about +-0.1, and the gap is above 0.4,
    so 128 games are enough.  The run is deterministic: the opponents' draws are keyed by the env's seed, the learner's by
    the generator's."""
    against_random = _mean_final_rank("random")
    against_search = _mean_final_rank("mcts")
    print("mean final rank: against random agents %.4f, against searches %.4f, gap %.4f"
          % (against_random, against_search, against_random - against_search))
    assert against_search < against_random - STRENGTH_MARGIN
