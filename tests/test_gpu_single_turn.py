"""One learner against the random agent on the GPU (crl_ttt_step_single / crl_blokus_step_single): bit-exact against the
numpy restatement of the header's contract (tests/ttt_ref.py, tests/blokus_ref.py), a learner that plays the random agent's
own draw against the oracle's rollout of each game, ragged and large batches, both vector envs replayed from a HIP graph, and the
outcome rates of a uniformly random TicTacToe learner."""
import numpy as np
import pytest
import torch

from tests import blokus_ref as R
from tests import ttt_ref
from tests import ttt_probes as TP
from tests.gpu_util import DEV, np_of as _np, same_ttt_state as _ttt_same_state

pytestmark = pytest.mark.gpu

TTT_CONFIGS = TP.INSTANCE_ROWS              # every <P, win table / 4 directions / 13 directions> instance of the kernel
TTT_IDS = TP.INSTANCE_IDS


def _ttt_pair(dims, K, P, B):
    from colosseumrl_amd.batched import TTTBatch
    from oracle import oracle as O
    return TTTBatch(dims, K, P, B, device=DEV), O.TTTState(dims, K, P, B)


def _ttt_compare(tb, st, seat, act, seed):
    seat_t = torch.from_numpy(seat).to(DEV)
    out = tb.step_single(seat_t, None if act is None else torch.from_numpy(act).to(DEV), seed)
    reward, done, winners, obs, valid = ttt_ref.step_single(st, seat, act, seed, ttt_ref.random_agent)
    torch.cuda.synchronize()
    _ttt_same_state(tb, st)
    assert np.array_equal(_np(out["reward"]), reward) and np.array_equal(_np(out["done"]), done)
    assert np.array_equal(_np(out["winners"]), winners)
    assert np.array_equal(_np(out["board"]), obs) and np.array_equal(_np(out["valid"]).view(np.uint32), valid)
    return done


@pytest.mark.parametrize("mixed", [False, True], ids=["fixed_seat", "mixed_seats"])
@pytest.mark.parametrize("dims,K,P", TTT_CONFIGS, ids=TTT_IDS)
def test_ttt_against_restatement(dims, K, P, mixed):
    B, seed = 37, 1234 + P                                          # ragged: not a multiple of 4 or 64
    tb, st = _ttt_pair(dims, K, P, B)
    rng = np.random.default_rng(P * 10 + mixed)
    seat = (rng.integers(0, P, size=B) if mixed else np.full(B, P - 1)).astype(np.int8)
    tb.reset()
    _ttt_compare(tb, st, seat, None, seed)
    n_done = 0
    for _ in range(18):
        act = TP.single_turn_actions(st, rng)                        # empty and occupied cells, passes, values out of range
        n_done += int(_ttt_compare(tb, st, seat, act, seed).sum())
    assert n_done > 0


@pytest.mark.parametrize("dims,K,P", [((4, 4), 4, 4), ((16,), 6, 7)], ids=["4x4k4p4", "16k6p7"])
def test_ttt_against_restatement_without_the_win_table(dims, K, P, monkeypatch):
    """Boards of at most 16 cells on a context without the table of winning masks (CRL_TTT_NO_WIN_TABLE makes crl_ttt_create
    skip it): the kernel's shift-and test instead of the lookup."""
    monkeypatch.setenv("CRL_TTT_NO_WIN_TABLE", "1")
    test_ttt_against_restatement(dims, K, P, True)


def _ttt_agent_action(tb, seed):
    return tb.sample(seed, advance=False).to(torch.int64)            # the random agent's draw at the learner's own counter


@pytest.mark.parametrize("dims,K,P", TTT_CONFIGS, ids=TTT_IDS)
def test_ttt_learner_as_agent_is_the_rollout(dims, K, P):
    from colosseumrl_amd.batched import TTTBatch
    from oracle import oracle as O
    B, seed = 301, 99 + P
    tb = TTTBatch(dims, K, P, B, device=DEV)
    seat = torch.from_numpy((np.arange(B) % P).astype(np.int8)).to(DEV)
    tb.reset()
    tb.step_single(seat, None, seed)
    for _ in range(20):
        tb.step_single(seat, _ttt_agent_action(tb, seed), seed)
    torch.cuda.synchronize()
    tc = _np(tb.tcount)
    occ, winner, to_move = _np(tb.occ).view(np.uint32), _np(tb.winner), _np(tb.to_move)
    for g in np.random.default_rng(0).choice(B, size=24, replace=False):
        ref = O.TTTState(dims, K, P, 1)
        O.ttt_rollout(ref, seed, int(g), int(tc[g]))
        assert np.array_equal(ref.occ[:, 0], occ[:, g]) and ref.winner[0] == winner[g] and ref.to_move[0] == to_move[g], g


def test_ttt_large_batch():
    from colosseumrl_amd.batched import TTTBatch
    from oracle import oracle as O
    dims, K, P, B, seed = (3, 3), 3, 2, 262144, 5
    tb = TTTBatch(dims, K, P, B, device=DEV)
    seat = torch.from_numpy((np.arange(B) % P).astype(np.int8)).to(DEV)
    tb.reset()
    tb.step_single(seat, None, seed)
    for _ in range(9):
        out = tb.step_single(seat, _ttt_agent_action(tb, seed), seed)
    torch.cuda.synchronize()
    tc = _np(tb.tcount)
    occ, board = _np(tb.occ).view(np.uint32), _np(out["board"])
    for g in np.random.default_rng(1).choice(B, size=48, replace=False):
        ref = O.TTTState(dims, K, P, 1)
        O.ttt_rollout(ref, seed, int(g), int(tc[g]))
        assert np.array_equal(ref.occ[:, 0], occ[:, g]), g
        bd = ref.board()[0].astype(np.int16)
        assert np.array_equal(np.where(bd >= 0, (bd - g % P) % P, -1), board[g]), g


# ------------------------------------------------------------------ Blokus
def _blk_pair(B):
    from colosseumrl_amd.batched import BlokusBatch
    from oracle import oracle as O
    return BlokusBatch(B, device=DEV), O.BlokusState(B)


def _blk_same_state(bb, st):
    for name in ("occ", "inv", "score", "round", "to_move", "tcount"):
        want = getattr(st, name)
        got = _np(getattr(bb, name)).view(want.dtype)
        assert np.array_equal(got, want), name


def _blk_compare(bb, st, seat, act, seed, rank):
    out = bb.step_single(torch.from_numpy(seat).to(DEV), None if act is None else torch.from_numpy(act).to(DEV), seed,
                         rank=rank)
    reward, done, winners, n_valid, ob, op, osc = R.blokus_step_single(st, seat, act, seed, rank=rank)
    torch.cuda.synchronize()
    _blk_same_state(bb, st)
    assert np.array_equal(_np(out["reward"]), reward) and np.array_equal(_np(out["done"]), done)
    assert np.array_equal(_np(out["winners"]), winners) and np.array_equal(_np(out["n_valid"]), n_valid)
    assert np.array_equal(_np(out["board"]), ob) and np.array_equal(_np(out["pieces"]), op)
    assert np.array_equal(_np(out["score"]), osc)
    return reward, done


@pytest.mark.parametrize("rank", [False, True], ids=["id", "rank"])
def test_blokus_against_restatement(rank):
    from oracle import oracle as O
    B, seed = 10, 4321                                               # ragged: not a multiple of 4
    bb, st = _blk_pair(B)
    rng = np.random.default_rng(7 + rank)
    seat = rng.integers(0, 4, size=B).astype(np.int8)
    _blk_compare(bb, st, seat, None, seed, rank)
    codes, n_done = set(), 0
    for _ in range(60):
        act = np.empty(B, np.int64)
        for b in range(B):
            one = R.blokus_one(st, b)
            n = int(O.blokus_valid(one, player=np.array([seat[b]], np.int8))[0][0])
            kind = rng.integers(0, 10)
            if rank:
                act[b] = int(rng.integers(-3, n + 3)) if kind < 9 else int(rng.choice([2 ** 31, -(2 ** 35), 2 ** 40]))
            elif kind == 0:
                act[b] = int(rng.choice([-1, -2, -(2 ** 40)]))       # pass
            elif kind == 1:
                act[b] = int(rng.integers(0, 336000))                # any dense id: placed as the reference does, or an error
            elif kind == 2:
                act[b] = int(rng.choice([R.BLOKUS_TOP, R.BLOKUS_TOP + 5, 2 ** 31, 2 ** 40]))   # BAD_ACTION
            elif kind == 3:
                act[b] = O.blokus_encode(int(rng.integers(0, 3)), 19, 19, 0, 4)   # a shift the small pieces lack: IndexError
            elif kind == 4:
                held = int(one.inv[0, seat[b]])
                gone = [p for p in range(21) if not (held >> p) & 1]
                act[b] = O.blokus_encode(gone[0] if gone else 0, 5, 5, 0, 0)      # ValueError once a piece is gone
            elif kind == 5:
                act[b] = 336000 + int(rng.integers(0, 1344000))      # an extended id
            else:
                ids = R.blokus_list(one, player=np.array([seat[b]], np.int8))
                act[b] = int(rng.choice(ids)) if len(ids) else -1    # a legal id
        reward, done = _blk_compare(bb, st, seat, act, seed, rank)
        codes |= set(int(r) for r in reward[reward < 0])
        n_done += int(done.sum())
    if not rank:
        assert codes == {-1, -2, -3}, codes
    assert n_done > 0


def test_blokus_learner_as_agent_is_the_rollout():
    from colosseumrl_amd.batched import BlokusBatch
    from oracle import oracle as O
    B, seed = 70, 31
    bb = BlokusBatch(B, device=DEV)
    seat = torch.from_numpy((np.arange(B) % 4).astype(np.int8)).to(DEV)
    bb.step_single(seat, None, seed)
    for _ in range(40):
        bb.step_single(seat, bb.sample(seed, advance=False).to(torch.int64), seed)
    torch.cuda.synchronize()
    assert int(_np(bb.tcount).min()) > 100                          # past the end of the first games
    tc = _np(bb.tcount)
    for g in np.random.default_rng(2).choice(B, size=10, replace=False):
        ref = O.BlokusState(1)
        O.blokus_rollout(ref, seed, int(g), int(tc[g]))
        for name in ("occ", "inv", "score", "round", "to_move"):
            assert np.array_equal(getattr(ref, name)[0], _np(getattr(bb, name))[g].view(getattr(ref, name).dtype)), (g, name)


def test_blokus_large_batch():
    from colosseumrl_amd.batched import BlokusBatch
    from oracle import oracle as O
    B, seed = 16384, 17
    bb = BlokusBatch(B, device=DEV)
    seat = torch.from_numpy((np.arange(B) % 4).astype(np.int8)).to(DEV)
    bb.step_single(seat, None, seed)
    for _ in range(6):
        out = bb.step_single(seat, bb.sample(seed, advance=False).to(torch.int64), seed)
    torch.cuda.synchronize()
    tc, n_valid, board = _np(bb.tcount), _np(out["n_valid"]), _np(out["board"])
    for g in np.random.default_rng(3).choice(B, size=12, replace=False):
        ref = O.BlokusState(1)
        O.blokus_rollout(ref, seed, int(g), int(tc[g]))
        assert np.array_equal(ref.occ[0], _np(bb.occ)[g].view(np.uint32)), g
        s8 = np.array([g % 4], np.int8)
        assert int(O.blokus_valid(ref, player=s8)[0][0]) == n_valid[g]
        assert np.array_equal(O.blokus_observe(ref, s8)[0][0], board[g])


# ------------------------------------------------------------------ vector envs
def _replay(make, actions_of, steps):
    """An env stepped eagerly and a twin replayed from a captured graph, fed the same actions: equal outputs."""
    eager, graphed = make(), make()
    o1, o2 = eager.reset(), graphed.reset()
    action = torch.zeros((eager.num_envs,), dtype=torch.int64, device=DEV)
    rng = np.random.default_rng(11)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    a = actions_of(eager, rng)
    action.copy_(a)
    with torch.cuda.stream(s):
        graphed.step(action)                                        # warm-up on a side stream, as torch.cuda.graph wants
    torch.cuda.current_stream().wait_stream(s)
    eager.step(a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = graphed.step(action)
    n_done = 0
    for _ in range(steps):
        a = actions_of(eager, rng)
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
    assert n_done > 0


def test_ttt_vector_env_graph_replay():
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    B = 4099
    seat = torch.from_numpy((np.arange(B) % 3).astype(np.int8))

    def make():
        return TicTacToeSinglePlayerVectorEnv((3, 5), 3, 3, B, seat=seat, seed=21, device=DEV)

    def actions(env, rng):
        return torch.from_numpy(rng.integers(-2, 16, size=B)).to(DEV)
    _replay(make, actions, 30)


@pytest.mark.parametrize("mode", ["id", "rank"])
def test_blokus_vector_env_graph_replay(mode):
    from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv
    B = 203

    def make():
        return BlokusSinglePlayerVectorEnv(B, seat=2, seed=9, list_cap=2048 if mode == "id" else 0, action=mode, device=DEV)

    def actions(env, rng):
        if mode == "rank":
            return torch.from_numpy(rng.integers(-1, 400, size=B)).to(DEV)
        # the first listed id of the state the eager twin is in (both are in the same state)
        ids = env.batch.valid_list(2048, player=env.seat)[1][:, 0]
        return ids.to(torch.int64)
    _replay(make, actions, 35)


def test_vector_env_seats_and_arguments():
    from colosseumrl_amd.vector import BlokusSinglePlayerVectorEnv, TicTacToeSinglePlayerVectorEnv
    with pytest.raises(ValueError):
        TicTacToeSinglePlayerVectorEnv(batch=8, seat=2, device=DEV)
    with pytest.raises(ValueError):
        BlokusSinglePlayerVectorEnv(8, seat=torch.tensor([0, 1, 2, 3, 4, 0, 1, 2], dtype=torch.int8), device=DEV)
    with pytest.raises(ValueError):
        BlokusSinglePlayerVectorEnv(8, action="index", device=DEV)
    env = TicTacToeSinglePlayerVectorEnv(batch=8, seat=1, device=DEV)
    obs = env.reset()
    torch.cuda.synchronize()
    assert (env.batch.to_move == 1).all() and (obs["board"] == 1).sum() == 8        # the opponent's first mark, relative
    with pytest.raises(ValueError):
        env.step(torch.zeros(8, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("seat", [0, 1])
def test_ttt_random_learner_rates(seat):
    """A uniformly random learner against the random agent on 3x3: first mover wins 58.5 %, second 28.8 %, 12.7 % draws
    (exact values of random play), over the first episode of each of 65,536 games."""
    from colosseumrl_amd.vector import TicTacToeSinglePlayerVectorEnv
    B = 65536
    env = TicTacToeSinglePlayerVectorEnv((3, 3), 3, 2, B, seat=seat, seed=2024, device=DEV)
    env.reset()
    valid = env.batch.valid_mask()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    first = torch.zeros(B, dtype=torch.int8, device=DEV)
    seen = torch.zeros(B, dtype=torch.bool, device=DEV)
    bits = 1 << torch.arange(9, device=DEV, dtype=torch.int32)
    for _ in range(6):
        free = (valid[:, None] & bits[None, :]) != 0
        score = torch.rand((B, 9), generator=gen, device=DEV).masked_fill(~free, -1.0)
        _, reward, done, info = env.step(score.argmax(dim=1).to(torch.int64))
        new = (done != 0) & ~seen
        first = torch.where(new, reward, first)
        seen |= new
        valid = info["valid"].clone()
    assert bool(seen.all())
    win, loss = float((first == 1).float().mean()), float((first == -1).float().mean())
    draw = float((first == 0).float().mean())
    w_want, l_want = (0.585, 0.288) if seat == 0 else (0.288, 0.585)
    assert abs(win - w_want) < 0.01 and abs(loss - l_want) < 0.01 and abs(draw - 0.127) < 0.01, (win, loss, draw)
