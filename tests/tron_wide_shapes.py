"""Shape tables of the Tron tests above 40x40 and at the dispatch edges, in one place: tests/test_gpu_tron_wide.py runs
the kernels over them, tests/test_tron_wide_host.py runs only the reference side (CPU oracle, numpy avoid loop) and checks
that every case goes through the resets its GPU twin relies on.  No torch, no GPU: importable by the CPU suite."""

ROLLOUT_SEED, ROLLOUT_FIRST = 123, 11    # (under this seed every game of the cases below that must reset does)
ROLLOUT_KERNELS = ("auto", "gquad", "global")
THRESHOLD_B = 130                # ragged: two workgroups of 64 games + 2 games of the lane-per-player kernel

# (N, P, T): the two sides of every comparison in tron_gquad_pays (colosseumrl_amd/csrc/tron.hip), one launch of T steps
ROLLOUT_THRESHOLDS = [
    (20, 4, 1), (20, 4, 2),                  # boards up to 20x20: a one-step launch only
    (40, 4, 18), (40, 4, 19),                # 21..40, rows of whole dwords: T <= 18
    (39, 4, 32), (39, 4, 33),                # 21..40, other rows: T <= 32
    (21, 3, 32), (21, 3, 33),
    (44, 4, 201),                            # four players up to 44x44: always
    (45, 4, 200), (45, 4, 201),              # 45..56: T <= 200
    (56, 4, 200), (56, 4, 201),
    (57, 4, 48), (57, 4, 49),                # above 56: T <= 48
    (56, 3, 56), (56, 3, 57),                # three players: 56 / 24
    (57, 3, 24), (57, 3, 25),
    (56, 2, 24), (56, 2, 25),                # one or two players: 24 / 14
    (57, 2, 14), (57, 2, 15),
    (57, 1, 14), (57, 1, 15),
]
# the cases of ROLLOUT_THRESHOLDS in which every game must finish an episode (boards of 44x44 and above)
THRESHOLD_RESET_MIN_N = 44

# (N, P, B, chunks): launches split so that state and counters carry over; five and more players run the lane-per-game
# global kernel under every flag, up to four both kernels
ROLLOUT_WIDE = [
    (41, 5, 130, (40, 3)),
    (41, 8, 130, (40,)),
    (64, 8, 70, (60,)),
    (100, 4, 70, (48, 49)),
    (100, 5, 70, (30, 31)),
    (128, 7, 40, (60,)),
    (181, 3, 40, (24, 25)),
    (181, 4, 40, (48, 49)),
    (181, 8, 33, (60,)),
    (181, 2, 33, (14, 15, 60)),
]

AVOID_T = 150
AVOID_NOISE_SMALL = 0.1
# avoid agents at noise 0.1 rarely die on a wide board: at this noise the host loop alone finishes at least B episodes
AVOID_NOISE_WIDE = 0.5
# (N, P, B): tron_rollout_avoid_kernel<1..4> / tron_rollout_avoid_game_kernel<5..8>; small boards have walls near on every side
AVOID_SMALL = [(4, 4, 33), (4, 2, 70), (5, 1, 33), (5, 4, 70), (7, 8, 33), (9, 5, 70), (13, 7, 33)]
AVOID_WIDE = [(41, 5, 70), (57, 4, 33), (64, 8, 70), (100, 3, 33), (128, 2, 70), (181, 7, 33), (181, 4, 70)]


def avoid_seed(N, P):
    return 4321 + 16 * N + P


AVOID_FIRST = 7
# one call across the split into launches of at most kTronLaunchMaxT = 16,383 steps
AVOID_SPLIT = dict(N=9, Ps=(3, 6), B=66, T=16383 + 21, seed=5, noise=0.1, first=3)
