"""The shared pieces of colosseumrl_amd/batched.py on the host: the statistics table of each stepper against its ctypes
struct and against the tensors the constructors have always allocated, the output-dict helper, the argument checkers at
their boundary values, and `_call` over a stub library."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from colosseumrl_amd import _native, batched
from colosseumrl_amd.batched import BlokusBatch, TronBatch, TTTBatch

I8, I16, I32, U8 = torch.int8, torch.int16, torch.int32, torch.uint8
CPU = torch.device("cpu")

# attribute -> (dtype, shape) at the (B, P) below, written out from the constructors' allocations
TRON_3_3 = [("tcount", I32, (3,)), ("tstep", I32, (3,)), ("n_episodes", I32, (3,)), ("win_count", I32, (3, 3)),
            ("len_sum", I32, (3,)), ("ret_sum", I32, (3, 3)), ("last_winners", U8, (3,)), ("last_len", I16, (3,)),
            ("_results", I32, (3, 9)), ("_packed", I16, (3, 8))]
TTT_3_2 = [("tcount", I32, (3,)), ("tstep", I32, (3,)), ("n_episodes", I32, (3,)), ("win_count", I32, (2, 3)),
           ("draw_count", I32, (3,)), ("len_sum", I32, (3,)), ("_results", I32, (3, 5))]
BLOKUS_3 = [("tcount", I32, (3,)), ("tstep", I32, (3,)), ("n_episodes", I32, (3,)), ("win_count", I32, (4, 3)),
            ("len_sum", I32, (3,)), ("score_sum", I32, (4, 3)), ("_results", I32, (3, 10))]


@pytest.mark.parametrize("cls,struct,B,P,want", [(TronBatch, _native.TronStats, 3, 3, TRON_3_3),
                                                 (TTTBatch, _native.TTTStats, 3, 2, TTT_3_2),
                                                 (BlokusBatch, _native.BlokusStats, 3, 4, BLOKUS_3)])
def test_stats_table_layout(cls, struct, B, P, want):
    assert cls.STATS_STRUCT is struct
    assert list(cls.STATS) == [name for name, _ in struct._fields_]
    spec = cls._stat_spec(B, P)
    assert [(k, dt, tuple(shape)) for k, (dt, shape) in spec.items()] == want
    # the struct built from such tensors carries their addresses field by field; reset_stats zeroes every one of them
    obj = cls.__new__(cls)
    obj.__dict__.update(batched._alloc(spec, CPU, torch.ones))
    obj._stat_steps = 7
    st = obj._stats()
    assert [getattr(st, name) for name, _ in struct._fields_] == [getattr(obj, k).data_ptr() for k in spec]
    obj.reset_stats()
    assert all(int(getattr(obj, k).abs().sum()) == 0 for k in spec)
    assert cls is not TronBatch or obj._stat_steps == 0


def test_a_table_that_misses_the_struct_is_refused():
    with pytest.raises(TypeError):
        class Short(batched._RolloutStepper):
            STATS_STRUCT = _native.TTTStats
            STATS = {k: v for k, v in TTTBatch.STATS.items() if k != "draw_count"}
    with pytest.raises(TypeError):
        class Swapped(batched._RolloutStepper):
            STATS_STRUCT = _native.BlokusStats
            STATS = dict(reversed(list(BlokusBatch.STATS.items())))


def test_out_dict():
    spec = {"area": (I32, (5, 3, 2)), "info": (U8, (5, 3))}
    fresh = batched._out_dict(None, spec, CPU)
    assert {k: (t.dtype, tuple(t.shape), t.device) for k, t in fresh.items()} == {k: (dt, sh, CPU) for k, (dt, sh) in spec.items()}
    assert list(fresh) == list(spec) and all(t.is_contiguous() for t in fresh.values())
    assert batched._out_dict(fresh, spec, CPU) is fresh
    extra = dict(fresh, more=torch.zeros(1))
    assert batched._out_dict(extra, spec, CPU) is extra
    with pytest.raises(ValueError, match="info"):
        batched._out_dict({"area": fresh["area"]}, spec, CPU)
    for bad in (torch.zeros((5, 3), dtype=I32), torch.zeros((5, 4), dtype=U8), torch.zeros((3, 5), dtype=U8).t(),
                torch.zeros((5, 3), dtype=U8, device="meta")):
        with pytest.raises(ValueError, match="info"):
            batched._out_dict({"area": fresh["area"], "info": bad}, spec, CPU)


def test_int_in():
    for ok in (1, 65535):
        assert batched._int_in("playouts", ok, 1, 65535) == ok
    for bad in (0, 65536, True, 2.0):
        with pytest.raises(ValueError, match="playouts"):
            batched._int_in("playouts", bad, 1, 65535)
    assert batched._int_in("max_steps", 0, 0, 65535) == 0
    for bad in (-1, 65536, False, None):
        with pytest.raises(ValueError, match="max_steps"):
            batched._int_in("max_steps", bad, 0, 65535)


def test_unit():
    for ok in (-0.0, 0, 0.5, 1, 1.0):
        got = batched._unit("noise", ok)
        assert isinstance(got, float) and got == ok
    for bad in (math.nan, "0.1", True, -1e-9, math.nextafter(1.0, 2.0), math.inf, None):
        with pytest.raises(ValueError, match="noise"):
            batched._unit("noise", bad)


def test_candidates():
    assert batched._candidates(None, 5, CPU, 16) == 1
    for cap in (16, 65535):
        assert batched._candidates(torch.zeros((5, 1), dtype=I32), 5, CPU, cap) == 1
        assert batched._candidates(torch.zeros((5, cap), dtype=I32), 5, CPU, cap) == cap
        for bad in (torch.zeros((5, cap + 1), dtype=I32), torch.zeros((5, 0), dtype=I32), np.zeros((5, 3), np.int32),
                    torch.zeros((5, 3), dtype=torch.int64), torch.zeros((4, 3), dtype=I32), torch.zeros((5,), dtype=I32),
                    torch.zeros((3, 5), dtype=I32).t(), torch.zeros((5, 3), dtype=I32, device="meta")):
            with pytest.raises(ValueError, match="candidates"):
                batched._candidates(bad, 5, CPU, cap)


def test_seat():
    ok = torch.zeros((5,), dtype=I8)
    assert batched._seat(None, 5, CPU) is None and batched._seat(ok, 5, CPU) is ok
    for bad in (torch.zeros((5,), dtype=I32), torch.zeros((4,), dtype=I8), np.zeros(5, np.int8), 0):
        with pytest.raises(ValueError, match="seat"):
            batched._seat(bad, 5, CPU)


def test_player_mask():
    assert batched._player_mask(None, 3, "sample_avoid") == 0b111
    assert batched._player_mask([], 3, "sample_avoid") == 0
    assert batched._player_mask([2, 0, 2], 3, "sample_avoid") == 0b101
    for bad in ([3], [-1], [0, 3]):
        with pytest.raises(ValueError, match="sample_avoid"):
            batched._player_mask(bad, 3, "sample_avoid")


def test_seed():
    assert batched._seed(-1) == 2 ** 64 - 1
    assert batched._seed(2 ** 64 + 5) == 5 and batched._seed(0) == 0 and batched._seed(2 ** 64 - 1) == 2 ** 64 - 1


def test_tron_step_single_checks_every_buffer_before_the_library():
    tb = TronBatch.__new__(TronBatch)
    tb.device, tb.B, tb.P = CPU, 5, 3
    good = {"actions": torch.zeros((3, 5), dtype=I8), "learner_action": torch.zeros((5,), dtype=torch.int64),
            "reward": torch.zeros((5,), dtype=I8), "done": torch.zeros((5,), dtype=U8), "terminal": torch.zeros((5,), dtype=U8)}
    for k, t in good.items():
        for bad in (torch.zeros((4,), dtype=t.dtype), t.to(I32)):
            with pytest.raises(ValueError, match="^" + k):
                tb.step_single(**dict(good, **{k: bad}))


@pytest.mark.parametrize("cls", [TronBatch, TTTBatch, batched.TTTBoards, BlokusBatch])
def test_a_cpu_device_is_refused_before_any_native_call(cls, monkeypatch):
    lib = _StubLib(0)                       # (with a device visible: the device argument alone must be refused)
    monkeypatch.setattr(_native, "require_gpu", lambda: lib)
    with pytest.raises(_native.NativeError, match=cls.__name__):
        cls(device="cpu")
    assert lib.calls == []


# ---- _call over a stub library (no device here: the stream query and the device guard are replaced)
class _StubLib:
    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def crl_stub_entry(self, *args):
        self.calls.append(args)
        return self.rc


class _Guard:
    depth = 0

    def __init__(self, dev):
        self.dev = dev

    def __enter__(self):
        _Guard.depth += 1

    def __exit__(self, *exc):
        _Guard.depth -= 1
        return False


@pytest.fixture
def stub(monkeypatch):
    stream = C.c_void_p(0x5EED)
    monkeypatch.setattr(batched, "_stream", lambda: stream)
    monkeypatch.setattr(batched, "_DevGuard", _Guard)

    def make(cls, rc):
        obj = cls.__new__(cls)
        obj.device, obj.B, obj._lib, obj._ctx = CPU, 7, _StubLib(rc), types.SimpleNamespace(handle="handle")
        return obj
    yield make, stream
    assert _Guard.depth == 0


@pytest.mark.parametrize("cls", [TronBatch, TTTBatch, batched.TTTBoards, BlokusBatch])
def test_call_passes_handle_batch_arguments_and_stream(cls, stub, monkeypatch):
    make, stream = stub
    obj = make(cls, 0)
    checked = []
    monkeypatch.setattr(batched, "check", lambda rc, what="": checked.append((rc, what)))
    assert obj._call("crl_stub_entry", 1, None, "x") is None
    assert obj._lib.calls == [("handle", 7, 1, None, "x", stream)]
    assert obj._call("crl_stub_entry") is None
    assert obj._lib.calls[1] == ("handle", 7, stream)
    assert checked == []                    # a zero return code never reaches check()


def test_call_raises_on_a_nonzero_return(stub):
    make, _ = stub
    obj = make(TronBatch, -1)
    with pytest.raises(_native.NativeError, match="crl_stub_entry"):
        obj._call("crl_stub_entry", 3)
    assert len(obj._lib.calls) == 1
