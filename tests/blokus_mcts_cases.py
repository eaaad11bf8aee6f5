"""The edge cases of the Blokus tree search (crl_blokus_mcts and the copy of its search in the seated agent), named once:
tests/test_blokus_mcts_edges_host.py shows from the restatement's counters that each case reaches what it is named for,
tests/test_gpu_blokus_mcts_edges.py compares every case with the restatement bit for bit, and
tests/test_gpu_blokus_mcts_agent_edges.py holds the agent to crl_blokus_mcts on the cases with a widening root.

A case is one launch: a set of rows (positions with their step counters and the first game id) and S, R, W, cexp and the
candidates or None.  Every case uses the seed 0x123456789ABCDEF (both key words nonzero), a first game id of 2^32 or more (the
game id is its low 32 bits) and nonzero step counters, one of each set's at 2^32 - 2.

The row sets, from tests/blokus_positions.py and the oracle:
  chain    the empty board, game id 4002: with W = 1 the tree is a chain that grows one ply per simulation until the game
           ends, after 73 plies with this id (the id matters: with 4001 the game is over after 64)
  deep     the empty board, game id 4004: with W = 2 and cexp = 0 the search follows what has won down one line, which is 73
           plies long after 220 simulations, and chooses between two children at depth 63 and below.  A chain has nothing to
           choose, so none of its outputs depends on what the backup leaves in the nodes past the 64th; this tree's do.
           (Of the ids 4000 .. 4019 at S = 260, 4004 has the most such choices; 9 of the 20 have none.)
  five     rows 0 and 11 of tiny_inventories(12), the row of late(24) whose mover has 8 actions, one whose mover must pass
           while another player can move, and a finished one: 5 is no multiple of 2 or 3 trees per workgroup
  tiny     the first two of `five`, tiny11 their second
  capped   the rows of late(24) whose mover has 1, 2, 4, 6 and 8 legal actions; every action there ends the game, so the
           root gets all L of them as children and nothing else grows.  The root widens at simulations 0, 1, 4, 9, ... whatever
           R and cexp are, so whether a rank probe wraps depends on the game id alone: 4183 is the first base id from 4100
           on at which the probes of all four rows with L >= 2 wrap
  cand     the first row of tiny_inventories(12) with 74 legal actions or more, twice
  six      the six positions of tests/test_gpu_blokus_mcts.py

`ref(name, b)` is the restatement's result and counters for row b of a case, computed once per process."""
import collections
import functools

import numpy as np

from tests import blokus_mcts_ref as M
from tests import blokus_positions as BP
from tests.blokus_ref import blokus_list, blokus_one

SEED = 0x123456789ABCDEF
ID_BASE = 1 << 32                          # first_env_id = ID_BASE + the game id of row 0
KEYS = ("ids", "visits", "value", "nodes", "best")
S_MAX = 1823
CAPPED_L = (1, 2, 4, 6, 8)
TREES_S = (415, 416, 571, 572, 884, 885)   # the last S with 4, 3, 2 trees per workgroup and the first with 3, 2, 1

FIVE = ("tiny0", "tiny11", "late8", "must_pass", "finished")
ROW_NAMES = {"chain": ("empty",), "deep": ("empty",), "five": FIVE, "tiny": FIVE[:2], "tiny11": FIVE[1:2], "capped": tuple("L%d" % n for n in CAPPED_L),
             "cand": ("all_legal", "mixed"), "six": ("empty", "plies12", "plies40", "must_pass", "finished", "tcount_wrap")}

Case = collections.namedtuple("Case", "name kind rows S R W cexp cand")
Rows = collections.namedtuple("Rows", "state tcount first_env_id")


def _mover_counts(st):
    return BP.counts(st)[np.arange(st.B), st.to_move & 3]


@functools.lru_cache(maxsize=None)
def rows(which):
    """the row set `which` -> Rows(oracle state, tcount uint32 [B], first_env_id); the rows are ROW_NAMES[which]"""
    from oracle import oracle as O
    tiny, late = BP.tiny_inventories(12), BP.late(24)
    n_late = _mover_counts(late)
    if which == "chain":
        return Rows(O.BlokusState(1), np.array([5], np.uint32), ID_BASE + 4002)
    if which == "deep":
        return Rows(O.BlokusState(1), np.array([5], np.uint32), ID_BASE + 4004)
    if which in ("five", "tiny", "tiny11"):
        # (of the rows whose mover must pass, the one in which the others have the fewest actions: the shortest playouts)
        must_pass = int(np.argmin(np.where(BP.late_kinds(late)[0] >= 1, BP.counts(late).sum(axis=1), 1 << 30)))
        st = BP.concat([BP.clone(tiny, [0, 11]), BP.clone(late, [int(np.flatnonzero(n_late == 8)[0]), must_pass]), BP.finished(1)])
        tcount = np.array([5, 2 ** 32 - 2, 13, 9, 3], np.uint32)
        assert _mover_counts(st).tolist()[2:] == [8, 0, 0] and BP.counts(st)[3].sum() > 0 and BP.counts(st)[4].sum() == 0
        if which == "tiny":
            return Rows(BP.clone(st, [0, 1]), tcount[:2], ID_BASE + 4000)
        if which == "tiny11":
            return Rows(BP.clone(st, [1]), tcount[1:2], ID_BASE + 4001)
        return Rows(st, tcount, ID_BASE + 4000)
    if which == "capped":
        st = BP.clone(late, [int(np.flatnonzero(n_late == n)[0]) for n in CAPPED_L])
        return Rows(st, np.array([3, 15, 16, 2 ** 32 - 2, 7], np.uint32), ID_BASE + 4183)
    if which == "cand":
        roomy = int(np.flatnonzero(_mover_counts(tiny) >= 74)[0])
        return Rows(BP.clone(tiny, [roomy, roomy]), np.array([2 ** 32 - 2, 21], np.uint32), ID_BASE + 4200)
    if which == "six":
        from tests import test_gpu_blokus_mcts as OLD
        assert tuple(OLD.NAMES) == ROW_NAMES["six"]
        return Rows(OLD._positions()[0], np.array([7, 5, 13, 9, 3, 2 ** 32 - 2], np.uint32), ID_BASE + 4300)
    raise KeyError(which)


CAND_UNPLAYABLE = (1, 2, 3, 4)             # columns of the mixed row: an illegal dense id, -1, 336000, a repeat of column 0


@functools.lru_cache(maxsize=None)
def candidates():
    """int32 [2, 64] for the rows of `cand`: 64 distinct legal ids; and a legal id, a dense id that is not legal, -1, 336000,
    the first id again and 59 further distinct legal ids, the last of them in column 63"""
    r = rows("cand")
    legal = [int(i) for i in blokus_list(blokus_one(r.state, 0))]
    assert len(legal) >= 74
    spread = [legal[(k * len(legal)) // 64] for k in range(64)]   # over the whole list: every piece the mover can play
    illegal = next(i for i in range(1000, 336000) if i not in set(legal))
    mixed = [legal[3], illegal, -1, 336000, legal[3]] + legal[5:64]
    cand = np.array([spread, mixed], np.int32)
    assert cand.shape == (2, 64) and len(set(spread)) == 64 and len(set(mixed)) == 63 and mixed[63] in legal
    return cand


def _cases():
    out = [Case("chain_R1", "chain", "chain", 110, 1, 1, 256, False),
           Case("chain_R4", "chain", "chain", 110, 4, 1, 256, False),
           Case("deep_W2", "chain", "deep", 220, 1, 2, 0, False)]
    out += [Case("trees_S%d" % S, "trees", "five", S, 1, 8, 256, False) for S in TREES_S]
    out += [Case("trees_S572_R3", "trees", "five", 572, 3, 8, 256, False)]
    out += [Case("smax_c256", "smax", "tiny", S_MAX, 1, 64, 256, False),
            Case("smax_c0", "smax", "tiny", S_MAX, 1, 64, 0, False),
            Case("smax_R4_c65535", "smax", "tiny11", S_MAX, 4, 64, 65535, False),
            Case("smax_W3", "smax", "tiny", S_MAX, 1, 3, 256, False)]
    out += [Case("capped_R%d_c%d" % (R, cexp), "capped", "capped", 120, R, 8, cexp, False) for R in (1, 5) for cexp in (256, 65535)]
    out += [Case("cand_R%d" % R, "cand", "cand", 200, R, 8, 256, True) for R in (1, 3)]
    out += [Case("dispatch_R%d" % R, "dispatch", "six", 24, R, 4, 256, False) for R in (3, 4)]
    return out


CASES = collections.OrderedDict((c.name, c) for c in _cases())
ROWS_OF = [(c.name, b) for c in CASES.values() for b in range(len(ROW_NAMES[c.rows]))]    # every (case, row), for parametrize


def trees_per_workgroup(S):
    """what the wave-per-tree mapping puts into one workgroup, from the header's three constants"""
    return min(M.TREE_LDS // ((S + 1) * M.NODE_BYTES + M.FIXED_BYTES), 4)


@functools.lru_cache(maxsize=None)
def ref(name, b, seed=SEED):
    """(ids, visits, value, nodes, best) of tests/blokus_mcts_ref.search for row b of the case `name`, and its counters"""
    c = CASES[name]
    r = rows(c.rows)
    count = {}
    out = M.search(blokus_one(r.state, b), c.S, c.R, c.W, c.cexp, seed, (r.first_env_id + b) & 0xFFFFFFFF, int(r.tcount[b]),
                   [int(x) for x in candidates()[b]] if c.cand else None, count)
    return out, count
