"""A Tron state turned by quarter turns -- TEST INFRASTRUCTURE for the rotation tests (tests/test_tron_rotate_host.py,
tests/test_gpu_tron_rotate.py).

The contract of every read-only Tron evaluator (include/colosseum_hip.h: crl_tron_territory, crl_tron_sample_avoid,
crl_tron_sample_territory, crl_tron_playout, crl_tron_mcts, crl_tron_mcts_territory) and of crl_tron_step without reset is
written in RELATIVE actions (forward / right / left of a player's direction), in player indices, and in draws keyed by (game,
counter, player): nothing in it names a row, a column or a compass direction.  So it is exactly equivariant under a quarter
turn of the board, and every output of those calls must be bit-identical on the turned state.  The kernels are not symmetric
under the turn (a board row is a lane or a word, a column is a bit), which is what makes the equality a test.

The map of ONE quarter turn (clockwise as the board is printed, y growing downwards):

    cell       (x, y)      ->  (N - 1 - y, x)                flat index  y N + x  ->  x N + (N - 1 - y)
    board      [N, N]      ->  np.rot90(board, k=-1)         (so that board'[y', x'] == board[y, x])
    direction  d           ->  (d + 1) mod 4                 (0 N, 1 E, 2 S, 3 W: north becomes east, ...)
    heads                      through the cell map, dead players' heads as well
    deaths                     unchanged (who killed whom is a matter of player indices)

k quarter turns are the map applied k times.  What is NOT assumed equivariant, and therefore outside these tests: the start
layout (nothing says that the turned start positions are the start positions of the turned board), so every entry that
resets a game -- crl_tron_step with auto-reset, the rollout entries -- is held by the differential tests only."""
import numpy as np


def rotate_cells(N, cells, k=1):
    """flat cell indices (any integer array) after k quarter turns, in the same dtype"""
    cells = np.asarray(cells)
    c = cells.astype(np.int64)
    for _ in range(k % 4):
        x, y = c % N, c // N
        c = x * N + (N - 1 - y)
    return c.astype(cells.dtype)


def rotate(N, board, heads, dirs, deaths, k=1):
    """(board [B, N*N], heads [P, B], dirs [P, B], deaths [P, B]) after k quarter turns: new arrays of the same dtypes and
    shapes; the arguments are not written"""
    board = np.asarray(board)
    B = board.shape[0]
    turned = np.rot90(board.reshape(B, N, N), k=-(k % 4), axes=(1, 2))
    dirs = np.asarray(dirs)
    return (np.ascontiguousarray(turned).reshape(B, N * N), rotate_cells(N, heads, k),
            ((dirs.astype(np.int64) + k) & 3).astype(dirs.dtype), np.array(deaths))


def rotate_state(st, k=1):
    """an oracle TronState after k quarter turns (a copy: counters and statistics are kept as they are)"""
    out = st.copy()
    out.board[...], out.heads[...], out.dirs[...], out.deaths[...] = rotate(st.N, st.board, st.heads, st.dirs, st.deaths, k)
    return out
