"""The reference side of tests/test_gpu_tron_wide.py, alone: the CPU oracle's rollout and the numpy avoid loop over the
shape tables of tests/tron_wide_shapes.py.  The GPU tests compare kernels with these bit for bit; that says little where
no game is ever reset (a wide board, a short launch), so the episode conditions the GPU tests rely on are asserted here,
where a table edit that loses them fails without a GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import tron_ref
from tests import tron_wide_shapes as S


def _oracle_rollout(N, P, B, chunks):
    sh, sd = O.tron_start_positions(N, P)
    st = O.TronState(N, P, B)
    O.tron_reset(st, sh, sd)
    for T in chunks:
        O.tron_rollout(st, S.ROLLOUT_SEED, S.ROLLOUT_FIRST, T, sh, sd, n_threads=8)
    return st


def test_tables_hold_what_the_kernel_dispatch_needs():
    """Both sides of every threshold of tron_gquad_pays, every player count above 40x40, and for the avoid agent every
    template instance of both kernels, boards below 15x15 and above 40x40."""
    th = set(S.ROLLOUT_THRESHOLDS)
    for N, P, T in [(20, 4, 1), (40, 4, 18), (39, 4, 32), (21, 3, 32), (45, 4, 200), (56, 4, 200), (57, 4, 48), (56, 3, 56),
                    (57, 3, 24), (56, 2, 24), (57, 2, 14), (57, 1, 14)]:
        assert (N, P, T) in th and (N, P, T + 1) in th, (N, P, T)
    assert (44, 4, 201) in th
    assert len(th) == len(S.ROLLOUT_THRESHOLDS)
    wide = {(N, P) for N, P, _, _ in S.ROLLOUT_WIDE}
    assert {P for N, P in wide if N > 40} >= {2, 3, 4, 5, 7, 8} and max(N for N, _ in wide) == 181
    assert all(B <= 130 for _, _, B, _ in S.ROLLOUT_WIDE) and S.THRESHOLD_B == 130
    avoid = S.AVOID_SMALL + S.AVOID_WIDE
    assert {P for _, P, _ in avoid} >= {1, 2, 3, 4, 5, 7, 8}         # (six players: tests/test_gpu_tron_avoid.py)
    assert all(N < 15 for N, _, _ in S.AVOID_SMALL) and all(N > 40 for N, _, _ in S.AVOID_WIDE)
    assert {B for _, _, B in avoid} == {33, 70}
    assert S.AVOID_SPLIT["T"] > 16383 and min(S.AVOID_SPLIT["Ps"]) <= 4 < max(S.AVOID_SPLIT["Ps"])


@pytest.mark.parametrize("N,P,T", S.ROLLOUT_THRESHOLDS)
def test_threshold_rollouts_reset_every_game(N, P, T):
    st = _oracle_rollout(N, P, S.THRESHOLD_B, (T,))
    assert int(st.tcount.min()) == T == int(st.tcount.max())
    if N >= S.THRESHOLD_RESET_MIN_N:
        assert st.n_episodes.min() >= 1


@pytest.mark.parametrize("N,P,B,chunks", S.ROLLOUT_WIDE)
def test_wide_rollouts_reset_every_game(N, P, B, chunks):
    st = _oracle_rollout(N, P, B, chunks)
    assert st.n_episodes.min() >= 1


@pytest.mark.parametrize("N,P,B", S.AVOID_SMALL + S.AVOID_WIDE)
def test_avoid_host_loop_finishes_episodes(N, P, B):
    """At the table's noise the numpy + oracle loop finishes at least B episodes in AVOID_T steps, on the wide boards too."""
    noise = S.AVOID_NOISE_WIDE if N > 40 else S.AVOID_NOISE_SMALL
    sh, sd = O.tron_start_positions(N, P)
    ref = tron_ref.HostLoop(N, P, B, sh, sd)
    ref.run(S.AVOID_T, S.avoid_seed(N, P), noise, S.AVOID_FIRST)
    assert ref.st.n_episodes.sum() >= B
    assert np.array_equal(ref.st.tcount, np.full(B, S.AVOID_T, ref.st.tcount.dtype))
