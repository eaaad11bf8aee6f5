"""Plain-Python restatement of crl_tron_sample_mcts_territory (include/colosseum_hip.h): the territory tree search as a seated
agent.  The contract is made of two that exist, and so is this module: the noise draw is territory_ref's (the Philox block
{g, c, p, TAG_TERRITORY} under the seed, `threshold`, `mulhi`), the search is tron_mcts_territory_ref.search on
tron_mcts_ref.pos_of's position.  No code is shared with the kernel."""
import numpy as np

from tests import rng_ref as RNG
from tests import territory_ref as TV
from tests import tron_mcts_ref as M
from tests import tron_mcts_territory_ref as T

_CODE = (0, 1, -1)                           # 0 forward, 1 right, 2 left in crl_tron_step's encoding


def agent_max_simulations(N, m):
    """S_agent of the header: m waves of the search's per-wave LDS in one 64 KB workgroup, and no more than S_max"""
    nwords = (N * N + 31) // 32
    return min(M.max_simulations(N), ((65536 // m) - 8 * nwords) // 16 - 1)


def sample(st, S, Vs=256, cexp=256, seed=0, first_env_id=0, noise=0.0, players=None, agent="random", model_noise=0.1,
           method="levels", tcount=None, into=None, info=None):
    """The call's actions int8 [P, B] on the oracle state `st` (never written, its counters included): rows of `players`
    (default: all) are written into `into` (default: zeros).  `info`: a dict whose 'noisy', 'searched', 'over' (live, not
    noisy, fewer than two alive: plays 0) and 'dead' grow by one per masked row, and whose 'picks' collects (b, p, a) of the
    searched rows."""
    N, P, B = st.N, st.P, st.B
    players = list(range(P)) if players is None else list(players)
    assert N <= 64 and players and 1 <= S <= agent_max_simulations(N, len(set(players)))
    tc = st.tcount if tcount is None else tcount
    act = np.zeros((P, B), np.int8) if into is None else into
    thr = RNG.threshold(noise)
    g = (first_env_id + np.arange(B, dtype=np.uint64)) & np.uint64(RNG.M32)
    for p in players:
        w = RNG.philox(g, np.asarray(tc, np.uint64), p, TV.TAG_TERRITORY, seed)
        noisy = w[0].astype(np.uint64) < np.uint64(thr)
        uniform = RNG.mulhi(w[1], 3)
        for b in range(B):
            a, what = 0, "dead"
            if st.deaths[p, b] == 0:
                root = M.pos_of(st, b)
                if noisy[b]:
                    a, what = int(uniform[b]), "noisy"
                elif P >= 2 and root.n_alive() < 2:
                    what = "over"                                # the search skips the position: best -1 plays 0
                else:
                    a = T.search(N, root, p, S, Vs, cexp, agent, model_noise, seed, int(g[b]), int(tc[b]), None, method)[3]
                    what = "searched"
                    if info is not None:
                        info["picks"].append((b, p, a))
            if info is not None:
                info[what] += 1
            act[p, b] = _CODE[a]
    return act


def new_info():
    return {"noisy": 0, "searched": 0, "over": 0, "dead": 0, "picks": []}
