"""HIP Tron kernels against the CPU oracle and the numpy restatements on boards above 40x40 and at the edges of the host-side
dispatch (shape tables: tests/tron_wide_shapes.py; their reference side alone: tests/test_tron_wide_host.py):
crl_tron_rollout on both sides of every threshold of tron_gquad_pays and on wide boards with 2..8 players, under the
library's choice and under both kernels it chooses between; crl_tron_rollout_avoid / crl_tron_sample_avoid for every player
count on boards below 15x15 and above 40x40, and across the split into launches of 16,383 steps; crl_tron_playout with rows
that span whole waves, bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_tron import _rollout_pair
from test_gpu_tron_avoid import STATS, _check_rollout_against_loops, _state, _stats, _tb
from test_gpu_tron_playout import _check_against_restatement
from tests import tron_ref
from tests import tron_wide_shapes as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kernel", S.ROLLOUT_KERNELS)
@pytest.mark.parametrize("N,P,T", S.ROLLOUT_THRESHOLDS)
def test_rollout_at_dispatch_thresholds(N, P, T, kernel):
    """One launch of T steps on either side of each comparison in tron_gquad_pays: the lane-per-player kernel on boards in
    global memory ("gquad") and the kernel the library takes instead (lane per game in global memory above 40x40, the LDS
    kernels below, which "global" replaces by the former), so both candidates are checked at the shape whichever "auto"
    takes.  Every state array and statistic against the oracle, bit for bit; from 44x44 every game has been reset."""
    ost = _rollout_pair(N, P, S.THRESHOLD_B, (T,), seed=S.ROLLOUT_SEED, first=S.ROLLOUT_FIRST, kernel=kernel)
    if N >= S.THRESHOLD_RESET_MIN_N:
        assert ost.n_episodes.min() >= 1


@pytest.mark.parametrize("kernel", S.ROLLOUT_KERNELS)
@pytest.mark.parametrize("N,P,B,chunks", S.ROLLOUT_WIDE)
def test_rollout_on_wide_boards(N, P, B, chunks, kernel):
    """Boards of 41x41..181x181: tron_rollout_gquad_kernel<2..4> above 50x50, tron_rollout_kernel<P> (lane per game, global
    memory) with three to eight players, split launches (state, RNG position and statistics carry over)."""
    ost = _rollout_pair(N, P, B, chunks, seed=S.ROLLOUT_SEED, first=S.ROLLOUT_FIRST, kernel=kernel)
    assert ost.n_episodes.min() >= 1


@pytest.mark.parametrize("N,P,B", S.AVOID_SMALL)
def test_rollout_avoid_small_boards(N, P, B):
    """Boards below 15x15 (walls near on every side) over tron_rollout_avoid_kernel<1, 2, 4> and
    tron_rollout_avoid_game_kernel<5, 7, 8>: fused == device loop == numpy + oracle loop."""
    fused = _check_rollout_against_loops(N, P, B, S.AVOID_T, seed=S.avoid_seed(N, P), noise=S.AVOID_NOISE_SMALL,
                                         first_env_id=S.AVOID_FIRST)
    assert int(fused.n_episodes.sum().item()) >= B          # (equal to the host loop's, which the CPU suite checks alone)


@pytest.mark.parametrize("N,P,B", S.AVOID_WIDE)
def test_rollout_avoid_wide_boards(N, P, B):
    """Boards above 40x40, at a noise at which the host loop finishes at least B episodes."""
    from oracle import oracle as O
    ref = tron_ref.HostLoop(N, P, B, *O.tron_start_positions(N, P))
    ref.run(S.AVOID_T, S.avoid_seed(N, P), S.AVOID_NOISE_WIDE, S.AVOID_FIRST)
    assert ref.st.n_episodes.sum() >= B
    _check_rollout_against_loops(N, P, B, S.AVOID_T, seed=S.avoid_seed(N, P), noise=S.AVOID_NOISE_WIDE, first_env_id=S.AVOID_FIRST)


@pytest.mark.parametrize("P", S.AVOID_SPLIT["Ps"])
def test_rollout_avoid_across_the_launch_split(P):
    """rollout_avoid(16,383 + 21) in ONE call: crl_tron_rollout_avoid sends it out as two launches (the lane-per-player
    kernel keeps a launch's counts in 14..16 bits), which must be the same rollout.  Against the device loop of sample_avoid
    + step(auto_reset=True), whose step outputs are recorded and turned into the statistics on the host: state, tcount,
    every statistic, results() against results_from_columns().  The twin here is the device loop, not the numpy + oracle
    loop: that one needs about 9 s for this many steps (1.09 s per 2,000), and the golden tests and the shorter cases above
    already tie the device loop to the reference."""
    c = S.AVOID_SPLIT
    N, B, T, seed, noise, first = c["N"], c["B"], c["T"], c["seed"], c["noise"], c["first"]
    fused, loop = _tb(N, P, B, first_env_id=first), _tb(N, P, B, first_env_id=first)
    fused.rollout_avoid(T, seed, noise)
    rews = torch.empty((T, P, B), dtype=torch.int8, device=loop.device)
    terms = torch.empty((T, B), dtype=torch.uint8, device=loop.device)
    wins = torch.empty((T, B), dtype=torch.uint8, device=loop.device)
    act = torch.zeros((P, B), dtype=torch.int8, device=loop.device)
    for t in range(T):
        rew, term, win = loop.step(loop.sample_avoid(seed, noise, out=act), auto_reset=True)
        rews[t].copy_(rew), terms[t].copy_(term), wins[t].copy_(win)
    torch.cuda.synchronize()
    for a, b in zip(_state(fused), _state(loop)):
        assert np.array_equal(a, b)
    assert np.array_equal(fused.tcount.cpu().numpy(), loop.tcount.cpu().numpy())
    assert (fused.tcount == T).all()
    assert torch.equal(fused.results(), fused.results_from_columns())
    assert torch.equal(fused.results_packed(), fused.results_packed_from_columns())   # (the low 16 bits of totals that wrapped)
    assert not fused.packed_rows_exact()
    # the statistics of the recorded loop: an episode ends at every terminal step
    rews, terms, wins = rews.cpu().numpy().astype(np.int64), terms.cpu().numpy() != 0, wins.cpu().numpy()
    steps = np.arange(1, T + 1)[:, None]
    end = np.where(terms, steps, 0)
    last = end.max(axis=0)                                             # step count at the last terminal step (0: none)
    prev = np.where(end < last[None, :], end, 0).max(axis=0)           # ... and at the one before
    want = dict(tcount=np.full(B, T), tstep=T - last, n_episodes=terms.sum(axis=0), len_sum=last, last_len=last - prev,
                ret_sum=rews.sum(axis=0), last_winners=np.where(last > 0, wins[np.maximum(last - 1, 0), np.arange(B)], 0),
                win_count=np.stack([(terms & (((wins >> p) & 1) != 0)).sum(axis=0) for p in range(P)]))
    assert set(want) == set(STATS)
    assert want["n_episodes"].min() >= 100 and terms[16383:].sum() >= 10    # episodes end on both sides of the split
    got = _stats(fused)
    for k in STATS:
        mask = (1 << (8 * got[k].dtype.itemsize)) - 1                  # (the device fields are 8, 16 and 32 bits wide)
        assert np.array_equal(got[k].astype(np.int64) & mask, want[k].astype(np.int64) & mask), k


@pytest.mark.parametrize("agent", ["random", "avoid"])
def test_playout_rows_that_span_waves(agent):
    """R = 130 playouts a row: a row covers two whole waves and parts of two more, and its outputs are summed by atomics
    across them -- every output against the restatement, bit for bit (tron_playout_kernel<3, *>).  B = 3 leaves one game
    beside the two out-of-range seats, so that game keeps its live seat; B = 7 adds the dead seat and a finished game."""
    case = (13, 3, agent, 0.1, "end", 0, True)
    played = _check_against_restatement(case, B=3, Rn=130, A=2, dead_seat=False)
    assert (played == 130).any()
    played = _check_against_restatement(case, B=7, Rn=130, A=2)
    assert (played == 130).sum() >= 4
