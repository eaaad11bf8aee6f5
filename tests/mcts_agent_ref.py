"""Restatement of the search agent of include/colosseum_hip.h ("the tree search as a seated agent": crl_ttt_sample_mcts /
_rollout_mcts / _step_single_mcts), written from the header's words: rules 1 to 5 over the draws of the tactical agent
(tests/ttt_ref.draws) and the plain-Python search (tests/mcts_ref.search).  No code is shared with the kernel.

``mcts_agent(S, R, cexp, noise)`` is an agent with the signature and ``.tag`` that the frames of tests/ttt_ref.py take
(`sample`, `rollout`, `step_single`), so the three entries are those frames with this agent."""
import functools

import numpy as np

from tests import mcts_ref as M
from tests import rng_ref as RNG
from tests import ttt_ref as TR


@functools.lru_cache(maxsize=None)
def _game(dims, K, P):
    return M.Game(dims, K, P)


def mcts_agent(S, R, cexp=256, noise=0.0, count=None):
    """the search agent with S simulations of R playouts, exploration cexp / 256, at noise level `noise`.  `count`: a dict
    whose 'searches' is added to (the plies that searched)."""
    thr = RNG.threshold(noise)

    def agent(dims, K, P, occ, to_move, seed, g, c, c2, tag):
        assert c2 is None and tag == RNG.CRL_TAG_TTT_TACTICAL          # the entries that are no playouts
        occ, tm = np.asarray(occ).astype(np.uint32), np.asarray(to_move).astype(np.int64)
        g, c = np.asarray(g, np.uint64) & np.uint64(RNG.M32), np.asarray(c, np.uint64) & np.uint64(RNG.M32)
        game = _game(tuple(int(d) for d in dims), int(K), int(P))
        E = TR.empties(dims, occ)
        u, v = TR.draws(seed, g, c, None, tag)                         # rule 2: the tactical agent's two words
        act = np.full(len(tm), -1, np.int8)
        for i in range(len(tm)):
            e = int(E[i])
            if not 0 <= tm[i] < P or e == 0:                           # rule 1: the pass, no draw
                continue
            if int(u[i]) < thr:                                        # rules 3, 4: a noisy ply
                cells = [cell for cell in range(game.n) if (e >> cell) & 1]
                act[i] = cells[(int(v[i]) * len(cells)) >> 32]
            else:                                                      # rule 5: best of crl_ttt_mcts, tcount = c, winner = -1
                act[i] = M.search(game, [int(x) for x in occ[:, i]], int(tm[i]), S, R, cexp, seed, int(g[i]), int(c[i]))[3]
                if count is not None:
                    count["searches"] = count.get("searches", 0) + 1
        return act
    agent.tag, agent.playout_tag = RNG.CRL_TAG_TTT_TACTICAL, None
    return agent
