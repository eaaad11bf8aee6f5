"""What every restatement under tests/ shares about random numbers: the Philox4x32-10 counter-based generator (Salmon et
al., SC'11) in its two forms, the key of a seed, the twelve domain tags of colosseumrl_amd/csrc/crl_common.hpp, the noise
threshold and the mulhi32 draw.  Test infrastructure; no code is shared with the kernels.

``philox`` is vectorised numpy, ``philox_int`` works on Python ints (for the scalar loops of the tree search, which make
thousands of calls).  tests/test_tron_avoid_host.py, test_territory_host.py and test_ttt_mcts_host.py hold both to
``oracle.philox4x32``."""
import math

import numpy as np

M32 = 0xFFFFFFFF

# the Philox domain tags (the fourth counter word), under the names and with the values of crl_common.hpp
TAGS = {
    "CRL_TAG_TRON": 0x54520000,
    "CRL_TAG_TRON_AVOID": 0x54410000,
    "CRL_TAG_TRON_TERRITORY": 0x54760000,
    "CRL_TAG_TTT": 0x54540000,
    "CRL_TAG_BLOKUS": 0x424C0000,
    "CRL_TAG_TTT_PLAYOUT": 0x54500000,
    "CRL_TAG_TTT_TACTICAL": 0x54630000,
    "CRL_TAG_TTT_TACTICAL_PLAYOUT": 0x54430000,
    "CRL_TAG_TTT_MCTS": 0x544D0000,
    "CRL_TAG_BLOKUS_PLAYOUT": 0x42500000,
    "CRL_TAG_TRON_PLAYOUT": 0x54700000,
    "CRL_TAG_TRON_AVOID_PLAYOUT": 0x54610000,
}
CRL_TAG_TRON_AVOID = TAGS["CRL_TAG_TRON_AVOID"]
CRL_TAG_TRON_TERRITORY = TAGS["CRL_TAG_TRON_TERRITORY"]
CRL_TAG_TTT = TAGS["CRL_TAG_TTT"]
CRL_TAG_BLOKUS = TAGS["CRL_TAG_BLOKUS"]
CRL_TAG_TTT_PLAYOUT = TAGS["CRL_TAG_TTT_PLAYOUT"]
CRL_TAG_TTT_TACTICAL = TAGS["CRL_TAG_TTT_TACTICAL"]
CRL_TAG_TTT_TACTICAL_PLAYOUT = TAGS["CRL_TAG_TTT_TACTICAL_PLAYOUT"]
CRL_TAG_TTT_MCTS = TAGS["CRL_TAG_TTT_MCTS"]
CRL_TAG_BLOKUS_PLAYOUT = TAGS["CRL_TAG_BLOKUS_PLAYOUT"]
CRL_TAG_TRON_PLAYOUT = TAGS["CRL_TAG_TRON_PLAYOUT"]
CRL_TAG_TRON_AVOID_PLAYOUT = TAGS["CRL_TAG_TRON_AVOID_PLAYOUT"]


def tag_hex(name):
    """the tag as the C sources spell it (without the u suffix)"""
    return "0x%08X" % TAGS[name]


def key(seed):
    """the Philox key {seed lo, seed hi}"""
    return [seed & M32, (seed >> 32) & M32]


def threshold(noise):
    """thr = min(2^32, ceil(noise * 2^32)), in 64 bits (crl_noise_threshold)"""
    return min(1 << 32, math.ceil(float(noise) * 4294967296.0))


def mulhi(w, n):
    """mulhi32: (w * n) >> 32 of uint32 words w (n a scalar or an array), as int64"""
    return ((np.asarray(w, np.uint64) * np.asarray(n, np.uint64)) >> np.uint64(32)).astype(np.int64)


def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (broadcast arrays or scalars, taken mod 2^32) under key(seed): four uint32 arrays."""
    m = np.uint64(M32)
    c = [np.asarray(x, dtype=np.uint64) & m for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = (np.uint64(k) for k in key(seed))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0 & m, p1 & m, n2 & m, p0 & m]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m
        k1 = (k1 + np.uint64(0xBB67AE85)) & m
    return [x.astype(np.uint32) for x in c]


def philox_int(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on Python ints (counters and key words already below 2^32): a tuple of four ints"""
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3
