"""The lane table of the lane-per-player byte kernel (csrc/tron_lane_table.hpp, read back through crl_tron_lane_table) against
a Python restatement of the slab layout: no GPU."""
import ctypes as C

import numpy as np
import pytest

from host_util import lib, tron_context
from oracle import oracle as O

RS, THREADS, WORDS, LUT_WORD, TABLE_WORDS = 24, 256, 12, 256 * 12, 256 * 12 + 24


def _table(h):
    n = lib().crl_tron_lane_table(h, None, 0)
    assert n == TABLE_WORDS
    buf = (C.c_uint32 * n)()
    assert lib().crl_tron_lane_table(h, buf, n) == n
    return np.frombuffer(buf, dtype=np.uint32).copy()


def _layout(N):
    """junk offset and stride of a slab: N + 2 rows of RS bytes, a junk dword, an odd number of dwords"""
    junk = (N + 2) * RS
    stride = (junk + 4) & ~3
    if (stride >> 2) % 2 == 0:
        stride += 4
    return junk, stride


@pytest.mark.parametrize("N,P", [(20, 4), (20, 2), (16, 4), (12, 3)])
def test_table_matches_the_slab_layout(N, P):
    sh, sd = ([int(x) for x in a] for a in O.tron_start_positions(N, P))
    with tron_context(N, P, sh, sd) as h:
        tab = _table(h)
    junk, stride = _layout(N)
    cells, walls = set(), set()                                  # dword offsets the copies / the wall stores write
    for t in range(THREADS):
        w = [int(x) for x in tab[t * WORDS:(t + 1) * WORDS]]
        lane, wave, p, slot = t & 63, t >> 6, t & 3, t >> 2
        mine = slot * stride
        for k in range(5):
            R = lane + 64 * k
            if R >= 16 * N:
                assert w[k] == 0xffffffff
                continue
            e, r = divmod(R, N)
            slab = (wave * 16 + e) * stride
            row, jb = w[k] & 0xffff, w[k] >> 16
            assert row == slab + (r + 1) * RS and jb == slab + junk
            assert slab + RS <= row and row + RS <= slab + (N + 1) * RS          # inside its own slab, between the wall rows
            for q in range(6):                                   # the six dwords the copy-in stores: no two lanes share one
                assert row + 4 * q not in cells
                cells.add(row + 4 * q)
        seated = p < P
        my_junk = mine + junk + p
        assert w[6] & 0xffff == my_junk
        fresh_h = mine + (sh[p] // N + 1) * RS + sh[p] % N if seated else my_junk
        assert w[5] & 0xffff == fresh_h and w[5] >> 16 == mine + RS + 4 * p
        for off in (w[6] >> 16, w[7] & 0xffff, w[7] >> 16):
            rel = off - mine
            assert 0 <= rel < RS or (N + 1) * RS <= rel < (N + 2) * RS             # wall rows of MY slab
            assert off % 4 == 0 and off not in walls
            walls.add(off)
        for i in range(2):
            j = p + 2 * i
            assert w[8 + i] == sum(0xff << (8 * c) for c in range(4) if 4 * j + c >= N)
        assert w[10] == ((int(sd[p]) << 3) | 0x100 if seated else 0) and w[11] == 0
    assert len(cells) == 64 * N * 6 and len(walls) == 64 * 12
    assert not (cells & walls)
    junk_dwords = {s * stride + junk for s in range(64)}
    assert not (junk_dwords & cells) and not (junk_dwords & walls)
    assert max(cells | walls | junk_dwords) + 4 <= 64 * stride
    # the action table: entry t = four base-3 digits of t as 2-bit codes 0, 1, 3 (first digit in the low bits)
    lut = tab[LUT_WORD:].view(np.uint8)
    for t in range(81):
        digits = (t // 27, (t // 9) % 3, (t // 3) % 3, t % 3)
        assert lut[t] == sum((a + (a >> 1)) << (2 * i) for i, a in enumerate(digits))
    assert not lut[81:].any()


def test_contexts_without_a_table_and_bad_arguments():
    with tron_context(21, 2, (0, 440), (0, 2)) as h:             # above 20x20: the kernel does not play it
        assert lib().crl_tron_lane_table(h, None, 0) == 0
    with tron_context(9, 5, (0, 1, 2, 3, 4), (0, 0, 0, 0, 0)) as h:                # more than four players
        assert lib().crl_tron_lane_table(h, None, 0) == 0
    with tron_context() as h:
        assert lib().crl_tron_lane_table(h, None, -1) == -1
        short = (C.c_uint32 * 4)(7, 7, 7, 7)
        assert lib().crl_tron_lane_table(h, short, 3) == TABLE_WORDS and short[3] == 7      # at most cap dwords are written
    assert lib().crl_tron_lane_table(None, None, 0) == -1
