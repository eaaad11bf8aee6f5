"""Launch plans and the C-API entry on the host: the extension builds and imports with its two functions, refuses wrong
arity and argument types, the bind entries refuse what the rollout entries refuse (same code, a message under the bind
entry's name), crl_rollout_launch checks T and the plan, and the steppers pick the ctypes form under CRL_NO_FASTCALL=1.
Every call here returns before any HIP call, so nothing needs a GPU."""
import ctypes as C
import os

import pytest

from colosseumrl_amd import _native
from tests.host_util import D, refused as _refused, tron_context, ttt_context

TRON_FLAGS = 2 | 4 | 8 | 16 | 32 | 64 | 128


def _tron_stats(null=None):
    fields = [n for n, _ in _native.TronStats._fields_]
    return _native.TronStats(*[None if n == null else 64 for n in fields])


@pytest.fixture
def tron():
    with tron_context(20, 4, (21, 38, 361, 378), (1, 2, 0, 3)) as h:
        yield _native.lib(), h


def _bind_tron(lib, h, B=67, first=2 ** 32 + 3, state=(D, D, D, D), stats=None, flags=0):
    plan = C.c_void_p()
    rc = lib.crl_tron_rollout_bind(h, B, first, *state, stats if stats is not None else _tron_stats(), flags, C.byref(plan))
    return rc, plan


def test_extension_is_built_and_exposes_both_functions():
    """build() (tests/conftest.py runs it where the library is missing) makes the extension next to the library"""
    import sysconfig
    built = os.path.join(_native.PKG_DIR, "_crl_fast" + sysconfig.get_config_var("EXT_SUFFIX"))
    assert os.path.exists(built), "run __graft_entry__.build() first: %s is missing" % built
    fast = _native.fast()
    assert fast is not None, "colosseumrl_amd._crl_fast did not import after build()"
    assert callable(fast.rollout_launch) and callable(fast.stream_wait_mapped)
    assert fast.ABI_VERSION == _native.CRL_ABI_VERSION
    assert os.path.dirname(os.path.abspath(fast.__file__)) == _native.PKG_DIR


def test_fast_entry_refuses_wrong_arity_and_types():
    fast = _native.fast()
    assert fast is not None
    for args in ((), (0, 1, 2), (0, 1, 2, 3, 4)):
        with pytest.raises(TypeError):
            fast.rollout_launch(*args)
    for args in ((), (0, 1, 2, 3), (0, 1, 2, 3, 1.0, 5)):
        with pytest.raises(TypeError):
            fast.stream_wait_mapped(*args)
    with pytest.raises(TypeError):
        fast.rollout_launch(plan=0, seed=1, T=0, stream=0)  # positional only
    for bad in (None, 1.5, "7", b"7", [1]):
        for i in range(4):
            args = [0, 1, 0, 0]
            args[i] = bad
            with pytest.raises(TypeError):
                fast.rollout_launch(*args)
        for i in range(5):
            args = [0, 0, 0, 1, 1.0]
            args[i] = bad
            if i == 4 and bad == 1.5:
                continue                                     # (a float IS a timeout)
            with pytest.raises(TypeError):
                fast.stream_wait_mapped(*args)
    with pytest.raises(OverflowError):
        fast.rollout_launch(0, 1, 2 ** 31, 0)


def test_fast_entry_hands_back_the_library_code(tron):
    """a refused call comes back as the return code, with the library's message in place; 64-bit arguments are masked, not
    refused"""
    lib, h = tron
    fast = _native.fast()
    assert fast.rollout_launch(0, 2 ** 64 - 1, 5, 0) == -1
    assert b"plan is NULL" in lib.crl_last_error()
    assert fast.stream_wait_mapped(0, 0, 0, 1, 0.5) == -1
    assert b"NULL flag pointer" in lib.crl_last_error()
    rc, plan = _bind_tron(lib, h)
    assert rc == 0 and plan.value
    try:
        assert fast.rollout_launch(plan.value, 2 ** 64 + 5, 0, 0) == 0       # T = 0: OK, nothing launched
        assert fast.rollout_launch(plan.value, -1, 0, 2 ** 64) == 0
        assert fast.rollout_launch(plan.value, 1, -1, 0) == -1
        assert b"T=-1" in lib.crl_last_error()
        with pytest.raises(_native.NativeError, match="T="):
            _native.check(fast.rollout_launch(plan.value, 1, (1 << 24) + 1, 0), "crl_rollout_launch")
    finally:
        assert lib.crl_rollout_unbind(plan) == 0


def test_tron_bind_refuses_what_the_rollout_refuses(tron):
    lib, h = tron
    name = b"crl_tron_rollout_bind"
    rc, plan = _bind_tron(lib, h, state=(None, D, D, D))                     # a NULL board
    _refused(lib, rc, name, b"NULL state pointer")
    assert plan.value is None
    for i in (1, 2, 3):
        state = [D] * 4
        state[i] = None
        _refused(lib, _bind_tron(lib, h, state=state)[0], name, b"NULL state pointer")
    rc, plan = _bind_tron(lib, h, state=(C.c_void_p(72), D, D, D))           # 20 x 20 = 400 cells: a whole number of 16 bytes
    _refused(lib, rc, name, b"16-byte aligned")
    assert plan.value is None
    for flags in (1, 256, 0x80000000, TRON_FLAGS | 1):
        _refused(lib, _bind_tron(lib, h, flags=flags)[0], name, b"unknown flags")
    for column in [n for n, _ in _native.TronStats._fields_]:
        rc, plan = _bind_tron(lib, h, stats=_tron_stats(null=column))
        if column in ("results", "packed"):                                   # the two optional rows
            assert rc == 0
            assert lib.crl_rollout_unbind(plan) == 0
        else:
            _refused(lib, rc, name, b"NULL stats pointer")
    for B in (0, -1, (1 << 31) + 1):
        _refused(lib, _bind_tron(lib, h, B=B)[0], name, b"B=")
    _refused(lib, _bind_tron(lib, None)[0], name, b"not a tron context")
    assert lib.crl_tron_rollout_bind(h, 67, 0, D, D, D, D, _tron_stats(), 0, None) == -1
    # every pin binds; 19 x 19 is not a whole number of 16 bytes and takes any board address
    for flags in (0, 2, 4, 8, 16, 32, 64, 128):
        rc, plan = _bind_tron(lib, h, flags=flags)
        assert rc == 0 and plan.value
        assert lib.crl_rollout_unbind(plan) == 0
    with tron_context(19, 4, (20, 36, 324, 340), (1, 2, 0, 3)) as h19:
        rc, plan = _bind_tron(lib, h19, state=(C.c_void_p(72), D, D, D))
        assert rc == 0
        assert lib.crl_rollout_unbind(plan) == 0


def test_the_old_entry_still_names_itself(tron):
    lib, h = tron
    rc = lib.crl_tron_rollout(h, 67, 1, 0, 5, None, D, D, D, _tron_stats(), 0, None)
    _refused(lib, rc, b"crl_tron_rollout:", b"NULL state pointer")
    rc = lib.crl_tron_rollout(h, 67, 1, 0, -1, D, D, D, D, _tron_stats(), 0, None)
    _refused(lib, rc, b"crl_tron_rollout:", b"T=-1")
    assert lib.crl_tron_rollout(h, 67, 1, 0, 0, D, D, D, D, _tron_stats(), 0, None) == 0


def test_launch_checks_t_and_the_plan(tron):
    lib, h = tron
    rc, plan = _bind_tron(lib, h)
    assert rc == 0
    try:
        assert lib.crl_rollout_launch(plan, 7, 0, None) == 0                # T = 0: OK, launches nothing
        for T in (-1, -(1 << 31), (1 << 24) + 1):
            _refused(lib, lib.crl_rollout_launch(plan, 7, T, None), b"crl_rollout_launch", b"T=")
    finally:
        assert lib.crl_rollout_unbind(plan) == 0
    _refused(lib, lib.crl_rollout_launch(None, 7, 5, None), b"crl_rollout_launch", b"plan is NULL")
    assert lib.crl_rollout_unbind(None) == 0                                 # harmless


def test_ttt_and_blokus_bind_checks():
    lib = _native.lib()
    with ttt_context(1, 3, 5, 3, 3) as h:
        def bind(ctx=h, B=131, state=(D, D, D), null=None):
            stats = _native.TTTStats(*[None if n == null else 64 for n, _ in _native.TTTStats._fields_])
            plan = C.c_void_p()
            return lib.crl_ttt_rollout_bind(ctx, B, 0, *state, stats, C.byref(plan)), plan
        for i in range(3):
            state = [D] * 3
            state[i] = None
            _refused(lib, bind(state=state)[0], b"crl_ttt_rollout_bind", b"NULL state pointer")
        for column in [n for n, _ in _native.TTTStats._fields_][:-1]:
            _refused(lib, bind(null=column)[0], b"crl_ttt_rollout_bind", b"NULL stats pointer")
        _refused(lib, bind(B=0)[0], b"crl_ttt_rollout_bind", b"B=")
        _refused(lib, bind(ctx=None)[0], b"crl_ttt_rollout_bind", b"tictactoe")
        rc, plan = bind(null="results")
        assert rc == 0
        assert lib.crl_rollout_launch(plan, 1, 0, None) == 0
        _refused(lib, lib.crl_rollout_launch(plan, 1, -3, None), b"crl_rollout_launch", b"T=-3")
        assert lib.crl_rollout_unbind(plan) == 0
        # a context of another game is refused by each bind entry
        plan = C.c_void_p()
        stats = _native.BlokusStats(*[64] * 7)
        _refused(lib, lib.crl_blokus_rollout_bind(h, 33, 0, D, D, D, D, D, stats, C.byref(plan)), b"crl_blokus_rollout_bind",
                 b"not a blokus context")
        _refused(lib, lib.crl_tron_rollout_bind(h, 33, 0, D, D, D, D, _tron_stats(), 0, C.byref(plan)), b"crl_tron_rollout_bind",
                 b"not a tron context")


def test_no_fastcall_selects_the_ctypes_form(monkeypatch):
    from colosseumrl_amd import batched
    lib = _native.lib()
    monkeypatch.delenv("CRL_NO_FASTCALL", raising=False)
    assert _native.fast() is not None
    assert batched._plan_launcher(lib) is _native.fast().rollout_launch
    monkeypatch.setenv("CRL_NO_FASTCALL", "1")
    assert _native.fast() is None
    launch = batched._plan_launcher(lib)
    assert launch is lib.crl_rollout_launch or launch.__name__ == "crl_rollout_launch"
    assert isinstance(launch, type(lib.crl_version))                          # a ctypes function pointer
    assert launch(None, 1, 5, None) == -1                                      # ... of the same entry
    assert b"plan is NULL" in lib.crl_last_error()
    monkeypatch.setenv("CRL_NO_FASTCALL", "0")                                 # only "1" switches it off
    assert _native.fast() is not None
