"""tron_rollout_quad_kernel behind its per-context lane table (csrc/tron_lane_table.hpp): the whole-wave prologue / epilogue
and today's ragged one in the same launch, seats without a player, every copy path, first game ids, rebinds, two contexts
alive at once, step counters that differ inside a wave -- bit for bit against the CPU oracle: board, heads, dirs, deaths, the
seven statistics columns (+ last_len) and both result rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
from backends import HipTron

SEED = 0xC0FFEE12345
STATE = ("board", "heads", "dirs", "deaths")
COLUMNS = ("tcount", "tstep", "n_episodes", "win_count", "len_sum", "ret_sum", "last_winners", "last_len")


class Pair:
    """a stepper of the library and the oracle's state of the same games, rolled out side by side"""

    def __init__(self, N, P, B, first=0):
        self.sh, self.sd = O.tron_start_positions(N, P)
        self.hip = HipTron(N, P, B, self.sh, self.sd)
        self.tb = self.hip.tb
        self.tb.first_env_id = first
        self.first = first
        self.ost = O.TronState(N, P, B)
        O.tron_reset(self.ost, self.sh, self.sd)

    def rollout(self, T, kernel="quad", seed=SEED, events=None):
        self.tb.rollout(T, seed, kernel=kernel, events=events)
        O.tron_rollout(self.ost, seed, self.first, T, self.sh, self.sd, n_threads=8)

    def check(self, what=""):
        import torch
        tb = self.tb
        for k in STATE + COLUMNS:
            want = getattr(self.ost, k)
            have = getattr(tb, k).cpu().numpy().view(want.dtype)
            assert np.array_equal(have, want), (k, what)
        assert torch.equal(tb.results(), tb.results_from_columns()), what
        assert torch.equal(tb.results_packed(), tb.results_packed_from_columns()), what


@pytest.mark.parametrize("T", [1, 4, 20, 33])
@pytest.mark.parametrize("B", [1, 16, 64, 65, 80, 1040])
def test_whole_and_ragged_waves(B, T):
    """20x20, four players: B = 80 and 1040 end in a workgroup whose first wave is whole and whose second is ragged or empty,
    65 in a wave of one game, 1 / 16 / 64 in a lone ragged / whole wave / whole workgroup; 33 steps cross the action refill."""
    pr = Pair(20, 4, B, first=123456)
    pr.rollout(T)
    pr.check()
    if T == 33:
        assert pr.ost.n_episodes.sum() > 0


@pytest.mark.parametrize("P", [2, 3])
def test_seats_without_a_player(P):
    pr = Pair(20, P, 80, first=7)
    pr.rollout(20)
    pr.rollout(33)
    pr.check()
    assert pr.ost.n_episodes.sum() > 0


@pytest.mark.parametrize("N", [16, 12, 19, 13, 7])
def test_other_copy_paths(N):
    """whole-dword rows that are not 20 wide (16, 12), rows at any alignment (19, 13), the byte path (7)"""
    pr = Pair(N, 4, 80, first=99)
    pr.rollout(20)
    pr.check()


def test_first_env_id_two_launches_and_rebind():
    pr = Pair(20, 4, 144, first=3 * 65536)
    pr.rollout(20)
    pr.rollout(20)                                              # the same plan again
    pr.check("two launches")
    pr.tb.first_env_id = pr.first = 5 * 65536 + 11              # drops the plan: the next launch binds a new one
    pr.rollout(20)
    pr.check("rebind")
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); e1.record()
    pr.rollout(4, events=(e0, e1))                              # crl_tron_rollout_timed
    torch.cuda.synchronize()
    pr.check("timed entry")


def test_two_contexts_alternating():
    """tables are per context: two steppers of different shapes, launched in turn"""
    a, b = Pair(20, 4, 80, first=1), Pair(16, 3, 96, first=2)
    for T in (20, 7, 20):
        a.rollout(T)
        b.rollout(T)
    a.check("20x20")
    b.check("16x16")


def test_step_counters_differ_inside_a_wave():
    """games enter with different step counters (the per-lane action countdown behind the new prologue)"""
    import torch
    pr = Pair(20, 4, 80, first=42)
    tc = (np.arange(80, dtype=np.uint32) * 7) % 45
    tc[16:32] = 31                                              # one whole wave shares a counter one step short of a refill
    pr.ost.tcount[:] = tc
    pr.tb.tcount.copy_(torch.from_numpy(tc.view(np.int32).copy()).view(pr.tb.tcount.dtype).to(pr.tb.device))
    pr.rollout(20)
    pr.rollout(33)
    pr.check()


def test_quad_pin_against_gquad_and_bytes():
    """the same input through the pinned quad kernel, the global-memory lane-per-player kernel and the lane-per-game byte kernel"""
    import torch
    runs = {}
    for kernel in ("quad", "gquad", "bytes"):
        pr = Pair(20, 4, 80, first=31337)
        pr.rollout(20, kernel=kernel)
        pr.rollout(33, kernel=kernel)
        pr.check(kernel)
        tb = pr.tb
        runs[kernel] = [getattr(tb, k).clone() for k in STATE + COLUMNS] + [tb.results(), tb.results_packed()]
    for kernel in ("gquad", "bytes"):
        for x, y in zip(runs["quad"], runs[kernel]):
            assert torch.equal(x, y), kernel
