"""The edge cases of the Blokus tree search (tests/blokus_mcts_cases.py) reach what they are named for.  These tests read the
table the GPU tests are parametrised with and the counters of the plain-Python restatement (tests/blokus_mcts_ref.py:
`search(..., count=...)`) -- not the kernels -- and fail when a case is taken out of the table or stops reaching its edge.
The conditions are conditions on the restatement alone, met by the inputs with room to spare (the figures beside them).

The restatement's share: the two chain cases 1.7 s and 4.4 s, the deep tree 2.8 s, an S = 1823 row 0.3 .. 1.6 s, every other row used here below
0.7 s; 23 s for the file."""
import math

import numpy as np
import pytest

from tests import blokus_mcts_cases as C
from tests import blokus_mcts_ref as M
from tests.blokus_ref import blokus_list, blokus_one

GROUP_R = 4                                # R >= this: one workgroup per tree ("the two mappings" of the contract)


def _children(out):
    return sum(1 for i in out[0] if i != -2)


def _legal(name, b):
    return [int(i) for i in blokus_list(blokus_one(C.rows(C.CASES[name].rows).state, b))]


def test_the_table():
    """every case the edges need, by what it is launched with"""
    got = {(c.kind, c.rows, c.S, c.R, c.W, c.cexp, c.cand) for c in C.CASES.values()}
    want = {("chain", "chain", 110, 1, 1, 256, False), ("chain", "chain", 110, 4, 1, 256, False),
            ("chain", "deep", 220, 1, 2, 0, False), ("trees", "five", 572, 3, 8, 256, False),
            ("smax", "tiny", 1823, 1, 64, 256, False), ("smax", "tiny", 1823, 1, 64, 0, False),
            ("smax", "tiny11", 1823, 4, 64, 65535, False), ("smax", "tiny", 1823, 1, 3, 256, False),
            ("cand", "cand", 200, 1, 8, 256, True), ("cand", "cand", 200, 3, 8, 256, True),
            ("dispatch", "six", 24, 3, 4, 256, False), ("dispatch", "six", 24, 4, 4, 256, False)}
    want |= {("trees", "five", S, 1, 8, 256, False) for S in (415, 416, 571, 572, 884, 885)}
    want |= {("capped", "capped", 120, R, 8, cexp, False) for R in (1, 5) for cexp in (256, 65535)}
    assert got == want and len(C.CASES) == len(want) == 22
    assert sorted(C.ROWS_OF) == sorted((c.name, b) for c in C.CASES.values() for b in range(C.rows(c.rows).state.B))
    assert C.S_MAX == M.S_MAX == 1823


def test_the_key_words_and_counters():
    """both seed words are nonzero, every first game id is 2^32 or more, so that the game id is its low word, and every step
    counter is nonzero with one of each launch at 2^32 - 2"""
    assert C.SEED >> 32 and C.SEED & 0xFFFFFFFF and C.SEED >> 32 != C.SEED & 0xFFFFFFFF
    for which in C.ROW_NAMES:
        r = C.rows(which)
        assert r.first_env_id >= 2 ** 32 and 0 < (r.first_env_id & 0xFFFFFFFF) < 2 ** 31
        assert r.tcount.dtype == np.uint32 and len(r.tcount) == r.state.B == len(C.ROW_NAMES[which])
        assert (r.tcount != 0).all() and (which in ("chain", "deep") or (r.tcount == 2 ** 32 - 2).sum() == 1)


@pytest.mark.parametrize("name", ["chain_R1", "chain_R4"])
def test_chain_is_deeper_than_a_wave(name):
    """W = 1: one child per node.  The backup walks more than 64 nodes, the children are gathered from more than 64, and
    once the game is over along the chain every simulation ends on the terminal node by selection.  (Measured: depth 73,
    deep 47, sel_term 37.)"""
    c = C.CASES[name]
    assert c.W == 1 and c.cexp == 256
    out, n = C.ref(name, 0)
    assert n["depth"] >= 68 and n["deep"] >= 20 and n["sel_term"] >= 20
    assert out[3] == n["depth"] + 1 > 64 and _children(out) == 1 and out[1][0] == c.S
    assert n["playouts"] == (c.S - n["sel_term"] - 1) * c.R         # (the node that ends the game has no playouts)


def test_deep_choices():
    """W = 2, cexp = 0: a line deeper than a wave on which the search chooses between two children whose n and w only the
    backup's second trip writes -- in a chain no output depends on them.  (Measured: depth 73, deep 45, deep_sel 111.)"""
    c = C.CASES["deep_W2"]
    assert (c.W, c.cexp, c.R) == (2, 0, 1)
    out, n = C.ref(c.name, 0)
    assert n["depth"] >= 68 and n["deep"] >= 20 and n["deep_sel"] >= 20
    assert _children(out) == 2 and sum(out[1]) == c.S and out[3] == c.S + 1 - n["sel_term"]
    assert C.ref("chain_R1", 0)[1]["deep_sel"] == 0


def test_chain_cases_differ_by_the_mapping_alone():
    a, b = C.CASES["chain_R1"], C.CASES["chain_R4"]
    assert a.R < GROUP_R <= b.R and a._replace(name="", R=0) == b._replace(name="", R=0)


def test_tree_counts():
    """the six S sit on the two sides of every step of trees per workgroup, and five rows fill no whole number of workgroups
    of two or three trees"""
    assert [C.trees_per_workgroup(S) for S in C.TREES_S] == [4, 3, 3, 2, 2, 1]
    assert C.trees_per_workgroup(C.S_MAX) == 1 and C.trees_per_workgroup(C.S_MAX + 1) == 0
    assert (C.S_MAX + 1) * M.NODE_BYTES + M.FIXED_BYTES == M.TREE_LDS          # at S_max the tree fills what there is
    B = C.rows("five").state.B
    assert B % 2 and B % 3 and B > 4
    assert C.CASES["trees_S572_R3"].R == GROUP_R - 1 and C.trees_per_workgroup(572) == 2


@pytest.mark.parametrize("name", [c.name for c in C.CASES.values() if c.kind == "trees"])
def test_tree_count_cases_fill_the_tree(name):
    """on a tiny row every simulation makes a node: node S, the last of the tree, is written"""
    c = C.CASES[name]
    assert C.ROW_NAMES[c.rows][:2] == ("tiny0", "tiny11")
    assert any(C.ref(name, b)[0][3] == c.S + 1 for b in (0, 1))


def test_smax_full_tree():
    """S = S_max, W = 64, cexp 256: 1,824 nodes, and the root as wide as it gets -- isqrt(1822) + 1 = 43 children on row 0,
    all 39 legal actions on row 11 -- with rank probes that wrap.  (Measured: wraps 4 and 6.)"""
    c = C.CASES["smax_c256"]
    assert (c.S, c.R, c.W, c.cexp) == (1823, 1, 64, 256)
    (out0, n0), (out11, n11) = C.ref(c.name, 0), C.ref(c.name, 1)
    assert out0[3] == out11[3] == 1824
    assert _children(out0) == 43 == math.isqrt(c.S - 1) + 1 and _children(out11) == 39 == len(_legal(c.name, 1))
    assert n0["wraps"] >= 1 and n11["wraps"] >= 1 and n11["full"] >= 1
    assert sum(out0[1]) == sum(out11[1]) == c.S


def test_smax_pure_exploitation():
    """cexp = 0: the search stays on what has won, and most simulations end on a terminal node by selection.  (Measured:
    1,248 and 1,663 of 1,823.)"""
    c = C.CASES["smax_c0"]
    assert (c.S, c.W, c.cexp) == (1823, 64, 0)
    for b in (0, 1):
        out, n = C.ref(c.name, b)
        assert n["sel_term"] > 1000 and out[3] == c.S + 1 - n["sel_term"]


def test_smax_workgroup_and_narrow():
    """the workgroup mapping at S_max with the largest cexp fills the tree; W = 3 keeps the root at three children"""
    c = C.CASES["smax_R4_c65535"]
    assert c.R == GROUP_R and c.cexp == 65535 and c.S == C.S_MAX
    out, n = C.ref(c.name, 0)
    assert out[3] == 1824 and _children(out) == 39 and n["wraps"] >= 1 and n["playouts"] % c.R == 0
    c = C.CASES["smax_W3"]
    for b in (0, 1):
        out, n = C.ref(c.name, b)
        assert _children(out) == 3 == c.W and sum(out[1]) == c.S == C.S_MAX


@pytest.mark.parametrize("name", [c.name for c in C.CASES.values() if c.kind == "capped"])
def test_capped_rows(name):
    """the root has all of its L >= 1 legal actions as children and no more: the cap c < max(L, 1) is what stops it (W = 8
    >= L, and 120 simulations would allow 11), and for L >= 2 a rank probe wraps from L - 1 to 0"""
    c = C.CASES[name]
    assert c.W >= max(C.CAPPED_L) and math.isqrt(c.S - 1) + 1 > max(C.CAPPED_L)
    for b, L in enumerate(C.CAPPED_L):
        out, n = C.ref(name, b)
        legal = _legal(name, b)
        assert len(legal) == L and n["full"] >= 1 and (L < 2 or n["wraps"] >= 1)
        assert _children(out) == L and sorted(out[0][:L]) == legal and out[0][L:] == [-2] * (c.W - L) and sum(out[1]) == c.S


def test_capped_cases_cover_both_mappings_and_the_largest_cexp():
    assert {(c.R >= GROUP_R, c.cexp) for c in C.CASES.values() if c.kind == "capped"} == {(False, 256), (False, 65535), (True, 256),
                                                                                         (True, 65535)}


@pytest.mark.parametrize("name", ["cand_R1", "cand_R3"])
def test_candidate_rows(name):
    """A = 64: slot 63 is a child.  Row 0: every column is one.  Row 1: the columns that cannot be played -- a dense id that
    is not legal, -1, 336000 and a repeat -- are -2 with no visits, the other 60 are children"""
    c = C.CASES[name]
    cand = C.candidates()
    legal = set(_legal(name, 0))
    assert cand.shape == (2, 64) and c.R < GROUP_R and len(legal) >= 74 and _legal(name, 1) == sorted(legal)
    out, _ = C.ref(name, 0)
    assert set(cand[0].tolist()) <= legal and len(set(cand[0].tolist())) == 64
    assert _children(out) == 64 and out[0] == cand[0].tolist() and out[0][63] >= 0 and out[1][63] >= 1 and min(out[1]) >= 1
    out, _ = C.ref(name, 1)
    bad = cand[1, list(C.CAND_UNPLAYABLE)].tolist()
    assert bad[0] not in legal and 0 <= bad[0] < 336000 and bad[1:3] == [-1, 336000] and bad[3] == cand[1, 0]
    for a in range(64):
        if a in C.CAND_UNPLAYABLE:
            assert out[0][a] == -2 and out[1][a] == 0 and out[2][a] == 0
        else:
            assert out[0][a] == cand[1, a] and cand[1, a] in legal and out[1][a] >= 1
    assert out[0][63] >= 0 and _children(out) == 60 and sum(out[1]) == c.S


def test_dispatch_cases_differ_by_the_mapping_alone():
    """R = 3 is the last value with a wave per tree, R = 4 the first with a workgroup per tree -- each wave plays exactly
    one playout -- on the same rows with everything else equal"""
    a, b = C.CASES["dispatch_R3"], C.CASES["dispatch_R4"]
    assert a.R == GROUP_R - 1 and b.R == GROUP_R and a._replace(name="", R=0) == b._replace(name="", R=0)
    assert C.rows("six").state.B == 6
