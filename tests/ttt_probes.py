"""One-ply probes of the TicTacToe win test: a numpy predicate that shares nothing with the kernels' shift-and test or the
oracle's line list, builders of hand-made states whose next ply completes a chosen mask, and the shape tables the host and
GPU tests walk (tests/test_ttt_probes_host.py, tests/test_gpu_ttt_probes.py, the single-turn and playout tests).

A board has at most 32 cells; cell (i, j, k) of a D0 x D1 x D2 board is bit (i * D1 + j) * D2 + k of a mask, boards of
fewer dimensions are padded with leading ones (tictactoe_2p_env.py:165-169 stores the board row-major)."""
import functools
import itertools

import numpy as np

RANDOM_MASKS = 50000                       # random masks per board of more than 16 cells (the lower bound of the sets)
MIN_PROBES = 16384                         # boards of at most 16 cells repeat their 2^n - 1 masks up to this many probes
MIN_WRAP_RUNS = 100                        # masks that hold a wrap run, per 2-D / 3-D board of more than 16 cells


def dims3(dims):
    return (1,) * (3 - len(dims)) + tuple(int(d) for d in dims)


def n_cells_of(dims):
    return int(np.prod(dims3(dims)))


def full_mask(dims):
    return (1 << n_cells_of(dims)) - 1


def directions():
    """the 13 canonical directions of a 3-D board: first non-zero component positive"""
    return [d for d in itertools.product((0, 1), (-1, 0, 1), (-1, 0, 1)) if d > (0, 0, 0)]


def unpack(dims, masks):
    """bool [N, D0, D1, D2]: the cells of each mask"""
    masks = np.asarray(masks, np.uint32)
    n = n_cells_of(dims)
    bits = (masks[:, None] >> np.arange(n, dtype=np.uint32)[None, :]) & np.uint32(1)
    return bits.astype(bool).reshape((len(masks),) + dims3(dims))


def pack(cells):
    """uint32 [N] from bool [N, ...]"""
    flat = cells.reshape(len(cells), -1).astype(np.uint64)
    return (flat << np.arange(flat.shape[1], dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def has_line(dims, K, masks):
    """bool [N]: the mask holds K cells in a row along an axis, a face diagonal or a space diagonal.  The board as an array,
    K slices of it offset along each direction and ANDed: no cell is ever given a linear index."""
    cells = unpack(dims, masks)
    shape = cells.shape[1:]
    hit = np.zeros(len(cells), bool)
    for d in directions():
        span = [shape[ax] - (K - 1) * abs(d[ax]) for ax in range(3)]
        if min(span) <= 0:
            continue                                            # no window of K fits along this direction
        run = np.ones((len(cells),) + tuple(span), bool)
        for s in range(K):
            sl = [slice(None)]
            for ax in range(3):
                lo = s * d[ax] if d[ax] >= 0 else (K - 1 - s) * -d[ax]
                sl.append(slice(lo, lo + span[ax]))
            run &= cells[tuple(sl)]
        hit |= run.any(axis=(1, 2, 3))
    return hit


def n_directions(dims, K):
    """directions along which a window of K fits: more than 4 selects the kernels' 13-direction instances"""
    shape = dims3(dims)
    return sum(1 for d in directions() if all(shape[ax] - (K - 1) * abs(d[ax]) > 0 for ax in range(3)))


# ---- mask sets
def _windows(dims, K):
    """every (direction, start cell): (cells of the K steps as coordinates or None where the walk leaves the board)"""
    shape = dims3(dims)
    for d in directions():
        for start in itertools.product(*(range(s) for s in shape)):
            walk = [tuple(start[ax] + s * d[ax] for ax in range(3)) for s in range(K)]
            yield d, start, walk, all(0 <= c[ax] < shape[ax] for c in walk for ax in range(3))


def _bit(shape, c):
    return 1 << ((c[0] * shape[1] + c[1]) * shape[2] + c[2])


def line_masks(dims, K):
    """every K-window that stays on the board, by walking coordinates"""
    shape = dims3(dims)
    return sorted({sum(_bit(shape, c) for c in walk) for _, _, walk, on in _windows(dims, K) if on})


def wrap_runs(dims, K):
    """K cells at the linear stride of a direction, from a start cell whose window along that direction leaves the board
    (cells 4, 5, 6 of a 3x5 board): what a wrong start mask would take for a line.  Runs that are a line of another
    direction of the same stride (on a board two cells wide, say) are left out."""
    shape = dims3(dims)
    n = n_cells_of(dims)
    out = set()
    for d, start, _, on in _windows(dims, K):
        stride = (d[0] * shape[1] + d[1]) * shape[2] + d[2]
        c0 = (start[0] * shape[1] + start[1]) * shape[2] + start[2]
        if on or stride <= 0 or c0 + (K - 1) * stride >= n:
            continue
        out.add(sum(1 << (c0 + s * stride) for s in range(K)))
    return sorted(out - set(line_masks(dims, K)))


def _random_masks(n, count, density, rng):
    """`count` non-zero masks, each of its own density drawn from the range"""
    got = np.zeros(0, np.uint32)
    while len(got) < count:
        dens = rng.uniform(density[0], density[1], size=count)
        m = pack(rng.random((count, n)) < dens[:, None])
        got = np.concatenate([got, m[m != 0]])
    return got[:count]


def mask_set(dims, K, rng, density=(0.15, 0.95)):
    """(masks uint32 [N], is_wrap bool [N]): every non-zero mask of a board of at most 16 cells (repeated up to MIN_PROBES
    probes); else every line, every line with one cell moved off it, every wrap run bare and under random extra cells,
    RANDOM_MASKS random masks of per-mask density out of `density`, and on 32 cells masks that hold bit 31."""
    n = n_cells_of(dims)
    if n <= 16:
        every = np.arange(1, 1 << n, dtype=np.uint32)
        masks = np.tile(every, -(-MIN_PROBES // len(every)))
        return masks, np.zeros(len(masks), bool)
    full = full_mask(dims)
    lines = line_masks(dims, K)
    moved = []
    for ln in lines:
        for c in range(n):
            if (ln >> c) & 1:
                rest = ln & ~(1 << c)
                moved += [rest | (1 << e) for e in range(n) if not (ln >> e) & 1]
    runs = wrap_runs(dims, K)
    wrap = list(runs)
    if runs:                                                    # each run again under sparse extra cells of the same player
        reps = -(-2 * MIN_WRAP_RUNS // len(runs))
        noise = _random_masks(n, reps * len(runs), (0.02, 0.25), rng)
        wrap += [int(r) | int(x) for r, x in zip(runs * reps, noise)]
    rand = _random_masks(n, RANDOM_MASKS, density, rng)
    parts = [np.array(lines, np.uint32), np.array(moved, np.uint32), np.array(wrap, np.uint32), rand]
    if n == 32:                                                 # the top bit: alone, on every line end, under random masks
        top = np.uint32(1 << 31)
        parts.append(np.array([1 << 31] + [ln | (1 << 31) for ln in lines], np.uint32))
        parts.append(rand[:4000] | top)
    masks = np.concatenate([p for p in parts if len(p)]).astype(np.uint32) & np.uint32(full)
    is_wrap = np.zeros(len(masks), bool)
    off = len(lines) + len(moved)
    is_wrap[off:off + len(wrap)] = True
    return masks, is_wrap


def one_ply_probes(dims, K, P, masks, rng):
    """Hand-made states one ply before `masks`: (occ uint32 [P, B], to_move int8 [B], action int8 [B], want bool [B]).
    The mover (spread over 0..P-1) holds masks[b] minus one of its bits, chosen at random, and plays that cell; the other
    players hold a random part of the complement -- nothing, all of it (the board becomes full) or anything between;
    no winner is recorded.  want[b] = the ply wins = masks[b] holds a line (it may have held one before the ply)."""
    masks = np.asarray(masks, np.uint32)
    B, n = len(masks), n_cells_of(dims)
    cells = unpack(dims, masks).reshape(B, n)
    assert cells.any(axis=1).all(), "a probe needs a cell to play"
    action = np.where(cells, rng.random((B, n)), -1.0).argmax(axis=1)
    if n == 32:                                                 # cell 31 as the action wherever the mask holds it, half the time
        top = cells[:, 31] & (rng.random(B) < 0.5)
        action[top] = 31
    to_move = (rng.permutation(B) % P).astype(np.int8)
    occ = np.zeros((P, B), np.uint32)
    occ[to_move, np.arange(B)] = masks & ~(np.uint32(1) << action.astype(np.uint32))
    if P > 1:
        kind = rng.integers(0, 4, size=B)                       # 0: nobody else, 1: the whole complement, else a random part
        dens = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, rng.random(B)))
        taken = ~cells & (rng.random((B, n)) < dens[:, None])
        owner = rng.integers(0, P - 1, size=(B, n))
        owner += owner >= to_move[:, None]                      # any player but the mover
        for p in range(P):
            occ[p] |= pack(taken & (owner == p))
    return occ, to_move, action.astype(np.int8), has_line(dims, K, masks)


def board_full_after(dims, occ, action):
    """bool [B]: the probe's ply fills the last empty cell"""
    after = np.bitwise_or.reduce(occ, axis=0) | (np.uint32(1) << action.astype(np.uint32))
    return after == np.uint32(full_mask(dims))


@functools.lru_cache(maxsize=None)
def probes_of(dims, K, P, density=(0.15, 0.95)):
    """the probe set of one row of PROBE_SHAPES, made once per process: dict of masks, is_wrap, occ, to_move, action, want"""
    rng = np.random.default_rng(n_cells_of(dims) * 1000 + K * 10 + P)
    masks, is_wrap = mask_set(dims, K, rng, density)
    occ, to_move, action, want = one_ply_probes(dims, K, P, masks, rng)
    out = dict(masks=masks, is_wrap=is_wrap, occ=occ, to_move=to_move, action=action, want=want,
               full=board_full_after(dims, occ, action))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_step_of(dims, K, P, density=(0.15, 0.95)):
    """the oracle's ply on probes_of(...), made once per process: dict of the state before (board) and after (occ, winner,
    to_move, board, valid) and the step outputs (reward, terminal, winners)"""
    from oracle import oracle as O
    pr = probes_of(dims, K, P, density)
    st = O.TTTState(dims, K, P, len(pr["masks"]))
    st.occ[:] = pr["occ"]
    st.to_move[:] = pr["to_move"]
    before = st.board()
    reward, terminal, winners = O.ttt_step(st, pr["action"])
    valid = np.uint32(full_mask(dims)) & ~np.bitwise_or.reduce(st.occ, axis=0)
    out = dict(board_before=before, occ=st.occ, winner=st.winner, to_move=st.to_move, board=st.board(), valid=valid,
               reward=reward, terminal=terminal, winners=winners)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- shape tables
# (dims, K, P, density range of the random masks): the four paths of the kernels' line test (K = 3, 4, 5 and the loop for
# K = 2, 6 and 7), 4- and 13-direction instances, 1-D / 2-D / 3-D, 32 cells, a single line (1x32 K 32) and none (3x5 K 6).
# The density range is narrowed where the default would leave one verdict rare: K = 2 wins on nearly every mask, a line
# of 7 or 32 needs a crowded board.
PROBE_SHAPES = [
    ((3, 3), 3, 2, None), ((3, 5), 3, 3, None), ((4, 4), 4, 2, None), ((2, 8), 2, 4, None), ((2, 8), 5, 3, None),
    ((16,), 6, 2, None), ((3, 5), 6, 2, None), ((2, 2, 2), 2, 5, None), ((2, 2, 4), 4, 3, None),
    ((5, 5), 4, 3, (0.15, 0.95)), ((5, 5), 5, 2, (0.15, 0.95)), ((4, 8), 4, 5, (0.15, 0.95)), ((4, 8), 5, 1, (0.15, 0.95)),
    ((6, 5), 6, 2, (0.15, 0.95)), ((3, 9), 3, 7, (0.15, 0.95)), ((32,), 7, 8, (0.15, 0.95)), ((1, 32), 32, 2, (0.5, 0.995)),
    ((3, 3, 3), 3, 4, (0.15, 0.95)), ((2, 4, 4), 2, 8, (0.02, 0.5)), ((2, 4, 4), 4, 3, (0.15, 0.95)),
    ((3, 3, 3), 2, 6, (0.02, 0.5)),
]
PROBE_SHAPES = [(d, k, p, dens or (0.15, 0.95)) for d, k, p, dens in PROBE_SHAPES]


def shape_id(dims, K, P):
    return "x".join(map(str, dims)) + "k%dp%d" % (K, P)


PROBE_IDS = [shape_id(d, k, p) for d, k, p, _ in PROBE_SHAPES]

# (dims, K, P) per kernel family and player count: the 24 + 24 instances of ttt_step_single_kernel / ttt_playout_kernel
TABLE_ROWS = [((2, 3), 2, 1), ((3, 3), 3, 2), ((3, 5), 3, 3), ((4, 4), 4, 4), ((2, 8), 5, 5), ((4, 4), 3, 6), ((16,), 6, 7),
              ((3, 5), 4, 8)]                                   # at most 16 cells, at most 4 directions: the win-mask table
ND4_ROWS = [((3, 6), 3, 1), ((5, 5), 5, 2), ((5, 5), 4, 3), ((6, 5), 6, 4), ((4, 8), 3, 5), ((2, 4, 4), 3, 6), ((32,), 7, 7),
            ((4, 7), 4, 8)]                                     # more than 16 cells, at most 4 directions
ND13_ROWS = [((3, 3, 3), 3, 1), ((2, 2, 2), 2, 2), ((2, 3, 2), 2, 3), ((3, 3, 3), 3, 4), ((2, 2, 8), 2, 5), ((3, 3, 3), 2, 6),
             ((2, 4, 4), 2, 7), ((3, 3, 3), 3, 8)]              # more than 4 directions (3-D, first dimension >= K)
INSTANCE_ROWS = TABLE_ROWS + ND4_ROWS + ND13_ROWS
INSTANCE_IDS = [shape_id(d, k, p) for d, k, p in INSTANCE_ROWS]


# (R with candidates, R without, candidate cells per game or None = every cell) of each row's playout case: sized so that the
# numpy restatement of a case takes about a second or less (the first four are the cases the suite had before the table)
PLAYOUT_SIZES = {
    "2x3k2p1": (16, 128, None), "3x3k3p2": (3, 100, None), "3x5k3p3": (1, 65, None), "4x4k4p4": (1, 10, None),
    "2x8k5p5": (1, 7, None), "4x4k3p6": (1, 13, None), "16k6p7": (1, 8, None), "3x5k4p8": (1, 12, None),
    "3x6k3p1": (4, 66, None), "5x5k5p2": (1, 10, 12), "5x5k4p3": (1, 65, None), "6x5k6p4": (1, 6, 8),
    "4x8k3p5": (1, 9, 10), "2x4x4k3p6": (1, 5, 6), "32k7p7": (1, 8, 10), "4x7k4p8": (1, 7, 12),
    "3x3x3k3p1": (5, 96, None), "2x2x2k2p2": (20, 130, None), "2x3x2k2p3": (6, 64, None), "3x3x3k3p4": (3, 1, None),
    "2x2x8k2p5": (4, 127, None), "3x3x3k2p6": (3, 66, None), "2x4x4k2p7": (2, 63, None), "3x3x3k3p8": (1, 4, 14),
}
PLAYOUT_CASES = [(row,) + PLAYOUT_SIZES[shape_id(*row)] for row in INSTANCE_ROWS]


def family_of(dims, K):
    """which of the three kernel families a shape runs (with the win table built)"""
    if n_directions(dims, K) > 4:
        return "nd13"
    return "table" if n_cells_of(dims) <= 16 else "nd4"


# ---- inputs that the host and the GPU tests of step_single and playout build alike (the host tests run the restatements
# alone on them and assert what the GPU tests rely on)
def single_turn_actions(st, rng):
    """int64 [B] learner actions for the oracle state `st`: mostly an empty cell, else a pass, an occupied cell or a value
    out of range"""
    bd = st.board()
    act = np.empty(st.B, np.int64)
    for b in range(st.B):
        empty = np.flatnonzero(bd[b] < 0)
        kind = rng.integers(0, 8)
        if kind == 0:
            act[b] = -1                                          # pass
        elif kind == 1 and (bd[b] >= 0).any():
            act[b] = int(rng.choice(np.flatnonzero(bd[b] >= 0)))  # occupied cell
        elif kind == 2:
            act[b] = int(rng.choice([st.n_cells, 127, -2, -129, 2 ** 33, -(2 ** 40)]))   # out of range
        else:
            act[b] = int(rng.choice(empty)) if len(empty) else -1
    return act


def random_positions(dims, K, P, B, rng):
    """B random positions: random plies from the empty board, some games played past their end (finished, not reset)"""
    from oracle import oracle as O
    st = O.TTTState(dims, K, P, B)
    for b in range(B):
        one = O.TTTState(dims, K, P, 1)
        for _ in range(int(rng.integers(0, one.n_cells + 1))):
            bd = one.board()[0]
            empty = np.flatnonzero(bd < 0)
            if len(empty) == 0 or (one.winner[0] >= 0 and rng.random() < 0.5):
                break
            O.ttt_step(one, np.array([rng.choice(empty)], np.int8))
        st.occ[:, b], st.winner[b], st.to_move[b] = one.occ[:, 0], one.winner[0], one.to_move[0]
    return st


def playout_candidates(n, B, rng, n_cand=None):
    """int64 [B, A] candidate cells: every cell (or n_cand random ones per game), -1, n and two random values, shuffled"""
    cells = np.tile(np.arange(n), (B, 1))
    if n_cand is not None:
        cells = rng.permuted(cells, axis=1)[:, :n_cand]
    cand = np.concatenate([cells, np.full((B, 1), -1), np.full((B, 1), n), rng.integers(-5, n + 40, size=(B, 2))], axis=1)
    return np.ascontiguousarray(rng.permuted(cand, axis=1))


def playout_case_inputs(cfg, B=67):
    """(st, tcount, cand-making rng, first_env_id, seed) of a playout test case: B is not a multiple of 64"""
    dims, K, P = cfg
    rng = np.random.default_rng(sum(dims) * 7 + P)
    first_env_id, seed = 1000 + P, 0xABCDEF0123 + P
    st = random_positions(dims, K, P, B, rng)
    tcount = rng.integers(0, 2 ** 32, size=B, dtype=np.uint64).astype(np.uint32)
    tcount[:3] = [0, 2 ** 32 - 3, 5]                              # a counter that wraps inside the playouts
    return st, tcount, rng, first_env_id, seed
