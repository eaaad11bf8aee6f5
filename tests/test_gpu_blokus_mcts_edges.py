"""crl_blokus_mcts at the edges of its tree layout, depth, width and key (tests/blokus_mcts_cases.py; what each case reaches
is shown by tests/test_blokus_mcts_edges_host.py): every row of every case bit-exact against the plain-Python restatement
(tests/blokus_mcts_ref.py) on all five outputs -- fewer than four trees per workgroup and a batch that fills no whole
number of workgroups, S = S_max = 1823, paths and child scans longer than a wave, nodes with all of their legal actions as
children, 64 candidates, R = 3 | 4, cexp = 0 and 65535, a seed with a high word and game ids past 2^32 -- and, on the GPU
alone, that a row does not depend on where it sits in such a batch, that the seed's high word is used and first_env_id's is
not, and that the state is only read.

Every launch and every restatement result is computed once.  The restatement's share per row: chain_R4 4.4 s, deep_W2
2.8 s, chain_R1 and the rows of the empty board and the game after 12 plies in the dispatch cases 1.7 .. 2.8 s, the must-pass row 0.5 .. 2 s as S
goes from 415 to 885, an S = 1823 row 0.3 .. 1.6 s, everything else below 1 s.  Beside an MI355X the slowest test,
chain_R1 with its restatement and the first launch, took 2.8 s and the 109 tests of the file 27 s."""
import functools

import numpy as np
import pytest

from tests import blokus_mcts_cases as C
from tests import blokus_positions as BP
from tests.gpu_util import blokus_batch, np_of, to_dev, u32_of

pytestmark = pytest.mark.gpu

STATE = ("occ", "inv", "score", "round", "to_move", "tcount")
PAD = 3


@functools.lru_cache(maxsize=None)
def _gpu(name, pad=0, seed=C.SEED, id_shift=0):
    """the launch of case `name` -> its five outputs by key, and 'read_only': the state is what it was.  pad: that many
    other rows in front, first_env_id lowered by as much (the rows keep their game ids; the outputs are those of the case's
    rows).  id_shift: added to first_env_id."""
    c = C.CASES[name]
    r = C.rows(c.rows)
    st, tcount = r.state, r.tcount
    if pad:
        st = BP.concat([BP.clone(C.rows("five").state, [2] * pad), st])
        tcount = np.concatenate([np.full(pad, 77, np.uint32), tcount])
    bb = blokus_batch(st, r.first_env_id - pad + id_shift, tcount)
    before = [u32_of(getattr(bb, k)).copy() for k in STATE]
    cand = to_dev(C.candidates()) if c.cand else None
    o = bb.mcts(c.S, c.R, cand, c.W, seed, c.cexp / 256.0)
    out = {k: np_of(o[k])[pad:].copy() for k in C.KEYS}
    out["read_only"] = all(np.array_equal(a, u32_of(getattr(bb, k))) for a, k in zip(before, STATE))
    return out


def _row(out, b):
    return tuple(out[k][b].tolist() for k in C.KEYS)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in C.KEYS)


@pytest.mark.parametrize("name,b", C.ROWS_OF, ids=["%s-%s" % (n, C.ROW_NAMES[C.CASES[n].rows][b]) for n, b in C.ROWS_OF])
def test_bit_exact(name, b):
    want, _ = C.ref(name, b)
    have = _row(_gpu(name), b)
    print(have, want)
    assert have == tuple(want)


@pytest.mark.parametrize("name", ["trees_S416", "trees_S571", "trees_S572", "trees_S884"])
def test_placement_with_two_and_three_trees(name):
    """five rows behind three others give what they gave.  With three trees per workgroup they move to the same waves of the
    next workgroups, which are now three (3 + 3 + 2 rows for 3 + 2); with two trees every row moves to the other wave."""
    assert C.trees_per_workgroup(C.CASES[name].S) in (2, 3)
    assert _same(_gpu(name, pad=PAD), _gpu(name))


def test_seed_high_word():
    """the same launch with bit 40 of the seed flipped: other draws, hence other children or visits, as in the restatement"""
    name, other = "capped_R1_c256", C.SEED ^ (1 << 40)
    got, base = _gpu(name, seed=other), _gpu(name)
    for b in range(len(C.CAPPED_L)):
        assert _row(got, b) == tuple(C.ref(name, b, other)[0])
    choice = [b for b, L in enumerate(C.CAPPED_L) if L >= 2]           # (with one legal action there is one tree)
    assert any(_row(got, b)[:2] != _row(base, b)[:2] for b in choice)
    assert any(C.ref(name, b, other)[0][:2] != C.ref(name, b)[0][:2] for b in choice)


def test_game_id_is_the_low_word():
    """first_env_id and first_env_id + 2^32 name the same games"""
    assert _same(_gpu("trees_S416", id_shift=1 << 32), _gpu("trees_S416"))
    assert _same(_gpu("chain_R1", id_shift=1 << 32), _gpu("chain_R1"))


@pytest.mark.parametrize("name", list(C.CASES))
def test_state_is_only_read(name):
    assert _gpu(name)["read_only"]
