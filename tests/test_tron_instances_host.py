"""The shape lists of the GPU tests of the Tron evaluators name every template instance their launchers dispatch on: the
player count P = 1 .. 8 (TRON_DISPATCH_P), the model agent where there is one, and for the floods the row word (N <= 32:
uint32_t, up to 64: uint64_t).  These tests read the lists the GPU tests are parametrised with -- not the kernels -- and fail
when a case is taken out so that an instance is launched by no test any more."""
import itertools

from tests import test_gpu_territory as TERR
from tests import test_gpu_tron_mcts as MC
from tests import test_gpu_tron_mcts_territory as MT
from tests import test_gpu_tron_playout as PO

PLAYERS = range(1, 9)
AGENTS = ("random", "avoid")


def _word(N):
    """the row word of the kernels that hold a board row in a lane's register"""
    assert N <= 64
    return 32 if N <= 32 else 64


def _agents(mark):
    """the agents a test module runs each of its shapes with"""
    name, values = mark.args
    assert name == "agent"
    return tuple(values)


def test_mcts_shapes_cover_every_instance():
    """tron_mcts_kernel<P, AVOID>: 16"""
    got = {(P, a) for (N, P), a in itertools.product(MC.SHAPES, _agents(MC.agents))}
    assert got == set(itertools.product(PLAYERS, AGENTS)) and len(got) == 16


def test_mcts_territory_shapes_cover_every_instance():
    """tron_mcts_territory_kernel<P, AVOID, W>: 32"""
    got = {(P, a, _word(N)) for (N, P), a in itertools.product(MT.SHAPES, _agents(MT.agents))}
    assert got == set(itertools.product(PLAYERS, AGENTS, (32, 64))) and len(got) == 32


def test_sample_territory_shapes_cover_every_instance():
    """tron_sample_territory_rows_kernel<P, W>: 16 (boards wider than 64 run the LDS kernel, which has its own cases), and
    tron_sample_territory_wide_kernel<P>: 8"""
    got = {(P, _word(N)) for N, P, B in TERR.SAMPLE_SHAPES if N <= 64}
    assert got == set(itertools.product(PLAYERS, (32, 64))) and len(got) == 16
    assert {P for N, P, B in TERR.SAMPLE_SHAPES if N > 64} == set(PLAYERS)


def test_playout_cases_cover_every_instance():
    """tron_playout_kernel<P, AVOID>: 16"""
    got = {(case[1], case[2]) for case in PO.CASES}
    assert got == set(itertools.product(PLAYERS, AGENTS)) and len(got) == 16
