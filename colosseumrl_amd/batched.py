"""Batched (vectorised) environment steppers: B independent games resident in HBM.

This is the new surface the reference does not have (it steps one Python state
per call): ``reset / step / rollout / observe`` over struct-of-arrays state held
in torch-ROCm tensors and advanced by the HIP kernels behind the C ABI
(include/colosseum_hip.h).  The single-state ``BaseEnvironment`` classes in
``colosseumrl_amd.envs`` are thin B=1 clients of these steppers.

No CPU path exists here: constructing a stepper without a visible MI355X raises.
"""
from typing import Optional, Sequence

import ctypes as C
import functools

import torch

from . import _native
from ._native import CRL_STEP_AUTO_RESET, CRL_STEP_RANK_ACTION, NativeError, check
from .envs.tron import layout as tron_layout


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's CURRENT stream of the current device as a hipStream_t.  (Through the raw-stream query where this torch has
    it: `torch.cuda.current_stream()` builds a Stream object per call, 1-2 us next to a 20 us launch.)"""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stream_handle() -> int:
    """`_stream()` as a plain int: what the plan launchers take (the C-API entry converts an int in a few nanoseconds; a
    ctypes c_void_p argument accepts one too)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _plan_launcher(lib):
    """The callable `(plan, seed, T, stream) -> rc` that launches a bound rollout plan, handles as ints: the C-API entry
    (colosseumrl_amd._crl_fast, csrc/fastcall.cpp) where it was built and imported, else ``crl_rollout_launch`` through
    ctypes (also with CRL_NO_FASTCALL=1: A/B runs and tests)."""
    fast = _native.fast()
    return fast.rollout_launch if fast is not None else lib.crl_rollout_launch


_ROLLOUT_KERNEL_FLAGS = {"auto": 0, "bits": _native.CRL_ROLLOUT_BITS, "bytes": _native.CRL_ROLLOUT_BYTES,
                         "global": _native.CRL_ROLLOUT_NO_LDS, "quad": _native.CRL_ROLLOUT_QUAD,
                         "qbits": _native.CRL_ROLLOUT_QBITS, "gquad": _native.CRL_ROLLOUT_GQUAD, "pair": _native.CRL_ROLLOUT_PAIR}


_STEP_KERNEL_FLAGS = {"auto": 0, "bytes": _native.CRL_STEP_BYTES, "staged": _native.CRL_STEP_STAGED}


class _DevGuard:
    """Makes `dev` the current device for a block, only when it is not already (torch's own context manager costs
    several microseconds per call, which is visible next to a 20-step rollout launch)."""
    __slots__ = ("dev", "prev")

    def __init__(self, dev):
        self.dev = dev.index
        self.prev = -1

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.dev:
            self.prev = cur
            torch.cuda.set_device(self.dev)

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
            self.prev = -1
        return False


def _want(t: torch.Tensor, dtype, shape, device, name):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s (got %s %s on %s)"
                         % (name, dtype, tuple(shape), device, t.dtype, tuple(t.shape), t.device))
    return t


def _seed(seed: int) -> int:
    """the seed as the C entries take it (uint64)"""
    return seed & (2 ** 64 - 1)


def _int_in(name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError("%s must be an int in [%d, %d], got %r" % (name, lo, hi, v))
    return v


def _unit(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) <= 1.0:       # (NaN fails the comparison)
        raise ValueError("%s must be a number in [0, 1], got %r" % (name, v))
    return float(v)


def _exploration(name: str, v) -> int:
    """cexp of crl_ttt_mcts: round(256 * v), in [0, 65535]"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) * 256.0 <= 65535.0:   # (NaN fails too)
        raise ValueError("%s must be a number in [0, %g], got %r" % (name, 65535 / 256, v))
    return int(round(256.0 * float(v)))


def _one_of(name: str, v, choices):
    if v not in choices:
        raise ValueError("%s must be %s, got %r" % (name, " or ".join(repr(c) for c in choices), v))
    return v


def _candidates(cand: Optional[torch.Tensor], B: int, device, max_a: int) -> int:
    """A of a playout / territory call, checked as the C entries check it (A in [1, max_a]: 65535 for crl_*_playout, 16 for
    crl_tron_territory); candidates int32 [B, A] or None (A = 1)."""
    if cand is None:
        return 1
    if not isinstance(cand, torch.Tensor) or cand.dim() != 2 or cand.shape[0] != B:
        raise ValueError("candidates must be an int32 tensor of shape (%d, A)" % B)
    A = int(cand.shape[1])
    if not 1 <= A <= max_a:
        raise ValueError("candidates must have 1..%d columns, got %d" % (max_a, A))
    _want(cand, torch.int32, (B, A), device, "candidates")
    return A


def _seat(seat: Optional[torch.Tensor], B: int, device):
    """seat int8 [B], or None (player 0)"""
    if seat is not None:
        if not isinstance(seat, torch.Tensor):
            raise ValueError("seat must be an int8 tensor of shape (%d,)" % B)
        _want(seat, torch.int8, (B,), device, "seat")
    return seat


def _player_mask(players, P: int, who: str) -> int:
    """bit p set for every player id in `players` (None: all P)"""
    if players is None:
        return (1 << P) - 1
    mask = 0
    for p in players:
        if not 0 <= int(p) < P:
            raise ValueError("%s: player %d out of range 0..%d" % (who, int(p), P - 1))
        mask |= 1 << int(p)
    return mask


def _alloc(spec: dict, device, make=torch.empty) -> dict:
    """a fresh dict of buffers; spec: name -> (dtype, shape)"""
    return {k: make(shape, dtype=dt, device=device) for k, (dt, shape) in spec.items()}


def _out_dict(out: Optional[dict], spec: dict, device) -> dict:
    """the output dict of a call: fresh, or `out` with every buffer checked"""
    if out is None:
        return _alloc(spec, device)
    for k, (dt, shape) in spec.items():
        if k not in out:
            raise ValueError("out lacks %r" % k)
        _want(out[k], dt, shape, device, "out[%r]" % k)
    return out


def _flat_mc_pick(value: torch.Tensor, played: torch.Tensor, ids: torch.Tensor):
    """int64 [B]: ids[b, a] of the greatest value among the played rows (ties: the lowest a), -1 where none was played"""
    value = torch.where(played > 0, value, torch.full_like(value, -1))
    best = torch.argmax(value, dim=1, keepdim=True)                      # (the first of equal maxima)
    pick = torch.gather(ids, 1, best).squeeze(1).to(torch.int64)
    return torch.where(played.amax(dim=1) > 0, pick, torch.full_like(pick, -1))


class _Ctx:
    """Owns one crl_ctx handle."""

    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        try:
            if self.handle:
                _native.lib().crl_destroy(self.handle)
                self.handle = None
        except Exception:  # interpreter shutdown
            pass


class _Stepper:
    """What every stepper class shares: how it is constructed (`_open`) and how it launches (`_call`)."""

    def _open(self, device, first_env_id: int, create: str, *args):
        """Resolves `device` (a ROCm device; the current one when no index is given), makes the context with the entry
        `create(*args, &handle)` and sets `_lib`, `_ctx` and `first_env_id`."""
        self._lib = _native.require_gpu()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NativeError("%s needs a ROCm device; there is no CPU path" % type(self).__name__)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        handle = C.c_void_p()
        with torch.cuda.device(self.device):     # (a context may keep tables on the device: TicTacToe's win masks do)
            check(getattr(self._lib, create)(*args, C.byref(handle)), create)
        self._ctx = _Ctx(handle)
        self.first_env_id = int(first_env_id)

    def _call(self, name: str, *args):
        """One launch: the entry `name(ctx, B, *args, stream)` on torch's CURRENT stream of the stepper's device, which is
        made current for the call only where it is not (`_DevGuard`)."""
        with _DevGuard(self.device):
            rc = getattr(self._lib, name)(self._ctx.handle, self.B, *args, _stream())
        if rc:
            check(rc, name)


class _Waitable:
    """``wait()``: block the host until everything queued so far on the stream the stepper launches on (torch's CURRENT
    stream of its device) has run -- the stream-scoped end of a rollout.  The wait is on MAPPED MEMORY
    (``crl_stream_wait_mapped``, include/colosseum_hip.h: a one-thread kernel behind the queued work publishes a sequence
    number into page-locked host memory, the host spins on it): ~3.5 us less than ``hipStreamSynchronize`` /
    ``torch.cuda.synchronize()`` behind a short launch (tools/ubench/mailbox_rtt.hip), which is a tenth of a 20-step
    rollout region.  Work on OTHER streams is not waited for (``torch.cuda.synchronize()`` does that)."""
    WAIT_TIMEOUT_S = 30.0            # after this long without the flag the call falls back to hipStreamSynchronize (and its error)
    _wait_flag = None

    def _open_wait(self):
        """Construction-time set-up of the completion channel: the flag word in mapped memory (a hipHostMalloc: ~1.3 ms, and the
        launches right behind a fresh mapping are slow) and one first wait, so that no rollout region ever pays for either --
        a stepper whose first `wait()` allocated lazily ran its NEXT region 6 us (35 us under a process group) slower."""
        import numpy as np
        from .single import HostBlob
        with torch.cuda.device(self.device):                   # the mapping is made for the stepper's device
            blob = HostBlob(self._lib, [("seq", np.uint32, 1)])
        self._wait_flag = (blob, blob.d["seq"], C.c_void_p(blob.v["seq"].ctypes.data))
        self._wait_seq = 0
        if not torch.cuda.is_current_stream_capturing():        # (a stepper built under graph capture: nothing may block there)
            self.wait()

    def wait(self):
        if self._wait_flag is None:
            self._open_wait()
            return
        self._wait_seq = seq = (self._wait_seq + 1) & 0xFFFFFFFF or 1
        with _DevGuard(self.device):
            rc = self._lib.crl_stream_wait_mapped(_stream(), self._wait_flag[1], self._wait_flag[2], seq, self.WAIT_TIMEOUT_S)
        if rc:
            check(rc, "crl_stream_wait_mapped")


def _per_game(B, P):
    return (B,)


def _per_player(B, P):
    return (P, B)


_STAT_ATTR = {"results": "_results", "packed": "_packed"}     # the two struct fields that are private attributes


class _RolloutStepper(_Stepper, _Waitable):
    """A stepper with fused rollouts: ``wait()`` and the rollout statistics.  A class lists its statistics columns ONCE, in
    `STATS`: column -> (dtype, shape as a function of (B, P)), in the order of the fields of `STATS_STRUCT`, the ctypes
    struct the C entries take by value (checked when the class is made).  The tensors (attributes of the column's name;
    ``_results`` / ``_packed`` for those two), `_stats()` and `reset_stats()` all come from that table."""
    STATS_STRUCT = None
    STATS = {}
    # Launch plans (include/colosseum_hip.h): `PLAN_BIND(ctx, B, first_env_id, *_state(), stats[, flags], &plan)` checks and
    # stores everything of a plain `rollout()` that does not change from call to call -- the tensors are never reallocated
    # --, so that a launch passes four scalars.  Bound at the first rollout (per kernel pin, for Tron), unbound with the
    # stepper.
    PLAN_BIND = None
    _plans = None                # flags (None where the entry has none) -> plan handle
    _launch = None               # `_plan_launcher`'s pick, made at the first bind

    def _bind_plan(self, flags=None) -> int:
        if self._plans is None:
            self._plans, self._launch = {}, _plan_launcher(self._lib)
        plan = C.c_void_p()
        check(getattr(self._lib, self.PLAN_BIND)(self._ctx.handle, self.B, self.first_env_id, *self._state(), self._stats(),
                                                 *(() if flags is None else (flags,)), C.byref(plan)), self.PLAN_BIND)
        self._plans[flags] = plan.value
        return plan.value

    def _rollout_plan(self, steps: int, seed: int):
        """`rollout` of the classes whose entry takes no flags: one launch through the plan"""
        plan = (self._plans and self._plans.get(None)) or self._bind_plan()
        with _DevGuard(self.device):
            rc = self._launch(plan, seed, int(steps), _stream_handle())
        if rc:
            check(rc, "crl_rollout_launch")

    def _unbind_plans(self):
        plans, self._plans = self._plans, None
        for plan in (plans or {}).values():
            self._lib.crl_rollout_unbind(plan)

    @property
    def first_env_id(self) -> int:
        return self._first_env_id

    @first_env_id.setter
    def first_env_id(self, value: int):
        """(a plan holds the id it was bound with: the next rollout binds again)"""
        self._first_env_id = int(value)
        self._unbind_plans()

    def __del__(self):
        try:
            self._unbind_plans()
        except Exception:  # interpreter shutdown
            pass

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        fields = [name for name, _ in cls.STATS_STRUCT._fields_]
        if list(cls.STATS) != fields:
            raise TypeError("%s.STATS lists %s, %s has %s" % (cls.__name__, list(cls.STATS), cls.STATS_STRUCT.__name__, fields))

    @classmethod
    def _stat_spec(cls, B: int, P: int) -> dict:
        """attribute -> (dtype, shape) of the statistics tensors of B games with P players"""
        return {_STAT_ATTR.get(k, k): (dt, shape(B, P)) for k, (dt, shape) in cls.STATS.items()}

    def _stat_tensors(self):
        return [getattr(self, _STAT_ATTR.get(k, k)) for k in self.STATS]

    def _stats(self):
        return self.STATS_STRUCT(*[t.data_ptr() for t in self._stat_tensors()])

    def reset_stats(self):
        for t in self._stat_tensors():
            t.zero_()


class TronBatch(_RolloutStepper):
    """B games of N x N Tron with P players (reference: envs/tron/TronGridEnvironment.py).

    State tensors (device):
      board  int8 [B, N*N]; heads int16 [P, B]; dirs int8 [P, B]; deaths int8 [P, B]
    """
    STATS_STRUCT = _native.TronStats
    PLAN_BIND = "crl_tron_rollout_bind"
    STATS = {"tcount": (torch.int32, _per_game), "tstep": (torch.int32, _per_game), "n_episodes": (torch.int32, _per_game),
             "win_count": (torch.int32, _per_player), "len_sum": (torch.int32, _per_game), "ret_sum": (torch.int32, _per_player),
             "last_winners": (torch.uint8, _per_game), "last_len": (torch.int16, _per_game),
             "results": (torch.int32, lambda B, P: (B, 3 + 2 * P)),               # packed by the rollout kernels
             # the same row in 16-bit fields (include/colosseum_hip.h, crl_tron_stats.packed): 16 bytes per game at P = 4
             "packed": (torch.int16, lambda B, P: (B, (4 + P + 1) & ~1))}

    def __init__(self, board_size: int = 19, num_players: int = 4, batch: int = 1, device="cuda",
                 ring_offset: int = 1, spawn_offset: int = 2,
                 start: Optional[Sequence[Sequence[int]]] = None, first_env_id: int = 0):
        self.N, self.P, self.B = int(board_size), int(num_players), int(batch)
        if start is None:
            start = tron_layout.start_positions(self.N, self.P, ring_offset, [spawn_offset] * self.P)
        self.start_heads = [int(h) for h in start[0]]
        self.start_dirs = [int(d) for d in start[1]]
        self._open(device, first_env_id, "crl_tron_create", self.N, self.P, (C.c_int16 * self.P)(*self.start_heads),
                   (C.c_int8 * self.P)(*self.start_dirs))
        dev, B, P, NN = self.device, self.B, self.P, self.N * self.N
        with torch.cuda.device(dev):
            self.board = torch.zeros((B, NN), dtype=torch.int8, device=dev)
            self.heads = torch.zeros((P, B), dtype=torch.int16, device=dev)
            self.dirs = torch.zeros((P, B), dtype=torch.int8, device=dev)
            self.deaths = torch.zeros((P, B), dtype=torch.int8, device=dev)
            self.rewards = torch.zeros((P, B), dtype=torch.int8, device=dev)
            self.terminal = torch.zeros((B,), dtype=torch.uint8, device=dev)
            self.winners = torch.zeros((B,), dtype=torch.uint8, device=dev)
            self.__dict__.update(_alloc(self._stat_spec(B, P), dev, torch.zeros))       # rollout bookkeeping
        self._stat_steps = 0                      # rollout steps the running totals span (since reset_stats)
        self._rollout_args = None
        self.reset()
        self._open_wait()

    def _state(self):
        return (_ptr(self.board), _ptr(self.heads), _ptr(self.dirs), _ptr(self.deaths))

    # -- new_state for all (or masked) games
    def reset(self, mask: Optional[torch.Tensor] = None):
        if mask is not None:
            _want(mask, torch.uint8, (self.B,), self.device, "mask")
        self._call("crl_tron_reset", _ptr(mask), *self._state())

    def reset_stats(self):
        super().reset_stats()
        self._stat_steps = 0

    # -- next_state for all games; actions int8 [P, B] in {0, +1, -1}
    def step(self, actions: torch.Tensor, auto_reset: bool = False, kernel: str = "auto"):
        """next_state of every game (``crl_tron_step``).  ``kernel``: "auto", "bytes" or "staged" -- all three run the one
        kernel (byte probes in HBM); "bytes" / "staged" are accepted for callers that pinned one of the two kernels it had."""
        _want(actions, torch.int8, (self.P, self.B), self.device, "actions")
        flags = (CRL_STEP_AUTO_RESET if auto_reset else 0) | _STEP_KERNEL_FLAGS[kernel]
        self._call("crl_tron_step", *self._state(), _ptr(actions), _ptr(self.rewards), _ptr(self.terminal),
                   _ptr(self.winners), flags)
        return self.rewards, self.terminal, self.winners

    def _bind_rollout(self):
        """the state / statistics arguments of the rollout entries: the tensors are never reallocated, so they are bound
        once, at the first rollout"""
        self._rollout_args = (*self._state(), self._stats())
        return self._rollout_args

    # -- T fused random-agent steps with auto-reset
    def rollout(self, steps: int, seed: int = 0, use_lds: bool = True, kernel: str = "auto", events=None):
        """``kernel``: "auto" (library's choice), "quad" / "pair" / "qbits" / "bits" / "bytes" (pin one of the LDS kernels), "gquad" / "global"
        (boards in global memory: one lane per player / per game);
        ``use_lds=False`` is the older spelling of "global".  All kernels give identical results.
        ``events``: an optional pair (start, stop) of ``torch.cuda.Event(enable_timing=True)`` -- either may be None -- that
        have been recorded at least once (torch creates the HIP event at the first record): the launch carries them in
        its dispatch (``crl_tron_rollout_timed``), so ``start.elapsed_time(stop)`` after a synchronise is the rollout's
        kernel time without marker packets around it."""
        flags = _ROLLOUT_KERNEL_FLAGS[kernel]
        if not use_lds:
            flags = _native.CRL_ROLLOUT_NO_LDS
        steps = int(steps)
        # `_call` written out: this launch is the benchmark's timed region, where one more Python frame per launch shows,
        # and the timed entry takes its events after the stream
        if events is None:
            plan = (self._plans and self._plans.get(flags)) or self._bind_plan(flags)
        else:
            args = self._rollout_args or self._bind_rollout()
        with _DevGuard(self.device):
            if events is None:                  # the plain launch: the bound plan, four scalars (the launcher masks the seed)
                rc = self._launch(plan, seed, steps, _stream_handle())
            else:
                if any(e is not None and not e.cuda_event for e in events):
                    raise ValueError("rollout(events=...): record() each event once before passing it (torch creates the "
                                     "HIP event lazily)")
                handles = [C.c_void_p(e.cuda_event) if e is not None else None for e in events]
                rc = self._lib.crl_tron_rollout_timed(self._ctx.handle, self.B, _seed(seed), self.first_env_id, steps, *args,
                                                      flags, _stream(), handles[0], handles[1])
        if rc:
            check(rc, "crl_rollout_launch" if events is None else "crl_tron_rollout_timed")
        self._stat_steps += steps

    def check_state(self) -> int:
        """Number of games whose state breaks the invariant of every reset / step / rollout product that the LDS
        rollout kernels rely on (heads on the board, ``board[heads[p]] == p + 1``); 0 unless states were hand-made.
        Synchronises."""
        bad = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._call("crl_tron_check_state", _ptr(self.board), _ptr(self.heads), _ptr(bad))
        return int(bad.item())

    # -- the rollout's random agent for one step: int8 [P][B] actions in the step() encoding
    def sample(self, seed: int = 0, advance: bool = True):
        """Actions the fused rollout would take at each game's step counter (``tcount``); with ``advance`` the counter
        moves on, so ``step(sample(seed), auto_reset=True)`` T times == ``rollout(T, seed)``.  Overwrite the rows of
        the players you control."""
        act = torch.empty((self.P, self.B), dtype=torch.int8, device=self.device)
        self._call("crl_tron_sample", _seed(seed), self.first_env_id, _ptr(self.tcount), int(advance), _ptr(act))
        return act

    # -- the reference's scripted opponent (SimpleAvoidAgent) for one step: int8 [P][B] actions in the step() encoding
    def sample_avoid(self, seed: int = 0, noise: float = 0.1, players=None, out: Optional[torch.Tensor] = None,
                     advance: bool = True):
        """Actions of the reference's ``SimpleAvoidAgent(noise)`` (envs/tron/rllib.py:68-95) at each game's step counter
        (``tcount``), under the Philox contract of ``crl_tron_sample_avoid`` (include/colosseum_hip.h), decided on the
        current (pre-step) boards.  ``players``: the player ids to fill (default: all); only their rows of ``out``
        (int8 [P, B]; a new zeroed tensor when None) are written, so a caller writes its learner's row and lets this fill
        in the opponents.  With ``advance`` the counter moves on, so ``step(sample_avoid(seed, noise), auto_reset=True)``
        T times == ``rollout_avoid(T, seed, noise)``."""
        return self._sample_scripted("sample_avoid", seed, noise, players, out, advance)

    def _sample_scripted(self, agent: str, seed, noise, players, out, advance):
        """`sample_avoid` / `sample_territory`: the entry crl_tron_<agent> for the rows of `players` in `out`"""
        mask = _player_mask(players, self.P, agent)
        if out is None:
            out = torch.zeros((self.P, self.B), dtype=torch.int8, device=self.device)
        else:
            _want(out, torch.int8, (self.P, self.B), self.device, "out")
        self._call("crl_tron_" + agent, _seed(seed), self.first_env_id, _ptr(self.tcount), int(advance), float(noise), mask,
                   *self._state(), _ptr(out))
        return out

    # -- batched playouts for one seat from every game's position (flat Monte Carlo's evaluation)
    def playout(self, playouts: int, candidates: Optional[torch.Tensor] = None, seed: int = 0, agent: str = "random",
                noise: float = 0.1, seat: Optional[torch.Tensor] = None, until: str = "end", max_steps: int = 0,
                out: Optional[dict] = None):
        """Playouts from every game's position, ONE launch (``crl_tron_playout``): row (b, a) plays first action
        ``candidates[b, a]`` (int32 [B, A]: 0 forward, 1 right, 2 left; any other value skips the row) for the seat
        ``seat[b]`` (int8 [B]; None: player 0) and then ``playouts`` games on private copies, every player on ``agent``
        ("random", or "avoid" with ``noise``).  ``candidates=None`` evaluates the position as it stands (A = 1).  A playout
        stops at the first terminal step; ``until="seat_done"`` also after the step in which the seat dies, ``max_steps``
        > 0 after that many steps.  The draws are keyed by ``seed``, the game ids and ``tcount`` as the counter base (the
        state is only read).  Returns {'wins' int32 [B, A, P], 'played', 'len_sum', 'ret_sum' int32 [B, A]} (``ret_sum``:
        the seat's summed rewards; skipped rows are zeros); ``out`` reuses such a dict.  No host synchronisation;
        capturable into a graph."""
        R = _int_in("playouts", playouts, 1, 65535)
        A = _candidates(candidates, self.B, self.device, 65535)
        if agent not in ("random", "avoid"):
            raise ValueError("agent must be 'random' or 'avoid', got %r" % (agent,))
        if until not in ("end", "seat_done"):
            raise ValueError("until must be 'end' or 'seat_done', got %r" % (until,))
        noise = _unit("noise", noise)
        _int_in("max_steps", max_steps, 0, 65535)
        _seat(seat, self.B, self.device)
        i32, BA = torch.int32, (self.B, A)
        out = _out_dict(out, {"wins": (i32, BA + (self.P,)), "played": (i32, BA), "len_sum": (i32, BA), "ret_sum": (i32, BA)},
                        self.device)
        flags = (_native.CRL_PLAYOUT_AVOID if agent == "avoid" else 0) | \
                (_native.CRL_PLAYOUT_UNTIL_SEAT_DONE if until == "seat_done" else 0)
        self._call("crl_tron_playout", _seed(seed), self.first_env_id, *self._state(), _ptr(self.tcount), _ptr(seat),
                   _ptr(candidates), A, R, noise, max_steps, _ptr(out["wins"]), _ptr(out["played"]), _ptr(out["len_sum"]),
                   _ptr(out["ret_sum"]), flags)
        return out

    @functools.cached_property
    def _moves3(self):
        """int32 [B, 3]: the three first actions [0, 1, 2] of every game (made at the first use)"""
        return torch.arange(3, dtype=torch.int32, device=self.device).expand(self.B, 3).contiguous()

    def flat_mc_action(self, playouts: int, seed: int = 0, agent: str = "random", noise: float = 0.1,
                       seat: Optional[torch.Tensor] = None, until: str = "end", max_steps: int = 0,
                       out: Optional[dict] = None) -> torch.Tensor:
        """Flat Monte Carlo for the seat in every game: ``playout`` on the three first actions [0, 1, 2], value = the mean
        ``ret_sum``, the best action (ties: the lowest) as int64 [B] in {0, 1, 2} for ``step_single``; -1 where every row
        was skipped (the seat is dead or the game is over).  ``out``: the playout dict to reuse.  No host
        synchronisation; capturable."""
        _int_in("playouts", playouts, 1, 65535)
        cands = self._moves3
        o = self.playout(playouts, cands, seed, agent, noise, seat, until, max_steps, out)
        # (returns go below -1: the pick compares mean returns shifted above _flat_mc_pick's -1 for unplayed rows)
        mean = o["ret_sum"].to(torch.float64) / float(playouts)
        return _flat_mc_pick(mean - mean.amin(dim=1, keepdim=True), o["played"], cands)

    # -- tree search for one seat; the contract is with crl_tron_mcts in include/colosseum_hip.h
    @functools.cached_property
    def mcts_max_simulations(self) -> int:
        """the most simulations ``mcts`` takes on this board (``crl_tron_mcts_max_simulations``: the tree, the path and the
        bitboards of a search stay in LDS); boards of 90x90 and more have no search and raise here"""
        rc = self._lib.crl_tron_mcts_max_simulations(self._ctx.handle)
        if rc < 0:
            check(rc, "crl_tron_mcts_max_simulations")
        return int(rc)

    def mcts(self, simulations: int, playouts: int = 16, seed: int = 0, exploration: float = 1.0, agent: str = "random",
             noise: float = 0.1, seat: Optional[torch.Tensor] = None, max_steps: int = 0, out: Optional[dict] = None):
        """A tree search (UCT) for the seat ``seat[b]`` (int8 [B]; None: player 0) in every game, ONE launch
        (``crl_tron_mcts``): each game builds a tree of its own over the SEAT's three actions by ``simulations`` descents (at
        most ``mcts_max_simulations``); the other players are part of the transition, played by ``agent`` ("random", or
        "avoid" with ``noise``) from counter-based draws, and each new leaf is valued by ``playouts`` (1 .. 1024) games of
        that agent that stop with the game, with the seat's death, or after ``max_steps`` > 0 steps.  ``exploration`` (0 ..
        65535 / 256; 0 = pure exploitation) multiplies sqrt(log2 n_parent / n_child) on a value scale of 0 .. 1.  The draws
        are keyed by ``seed``, the game ids and ``tcount`` as the counter base (the call reads the state and writes none of
        it).  Returns {'visits', 'value' int32 [B, 3]: simulations through the root's child at each action (0 forward, 1
        right, 2 left) and the seat's half-points there (2 per playout the seat survives as a winner, 1 per playout the
        cap stopped with the seat alive), 'nodes' int32 [B], 'best' int32 [B]: the most visited action (ties: the larger
        value, then the lower action; -1 where the seat is dead or the game is over)}; ``out`` reuses such a dict.  The
        visit counts are the policy target of an AlphaZero-style trainer.  No host synchronisation; capturable into a
        graph."""
        S = _int_in("simulations", simulations, 1, self.mcts_max_simulations)
        R = _int_in("playouts", playouts, 1, 1024)
        cexp = _exploration("exploration", exploration)
        _one_of("agent", agent, ("random", "avoid"))
        noise = _unit("noise", noise)
        _int_in("max_steps", max_steps, 0, 65535)
        _seat(seat, self.B, self.device)
        i32 = torch.int32
        out = _out_dict(out, {"visits": (i32, (self.B, 3)), "value": (i32, (self.B, 3)), "nodes": (i32, (self.B,)),
                              "best": (i32, (self.B,))}, self.device)
        self._call("crl_tron_mcts", _seed(seed), self.first_env_id, *self._state(), _ptr(self.tcount), _ptr(seat), S, R, cexp,
                   noise, max_steps, _ptr(out["visits"]), _ptr(out["value"]), _ptr(out["nodes"]), _ptr(out["best"]),
                   _native.CRL_PLAYOUT_AVOID if agent == "avoid" else 0)
        return out

    def mcts_action(self, simulations: int, playouts: int = 16, seed: int = 0, exploration: float = 1.0, agent: str = "random",
                    noise: float = 0.1, seat: Optional[torch.Tensor] = None, max_steps: int = 0,
                    out: Optional[dict] = None) -> torch.Tensor:
        """``mcts``'s most visited action as an int64 [B] action for ``step_single`` (-1 where the seat is dead or the game
        is over): the arg-max is the kernel's own ``best``, only widened here.  No host synchronisation; capturable."""
        return self.mcts(simulations, playouts, seed, exploration, agent, noise, seat, max_steps, out)["best"].to(torch.int64)

    # -- the same search with Voronoi territory at the leaves; the contract is with crl_tron_mcts_territory
    def mcts_territory(self, simulations: int, seed: int = 0, exploration: float = 1.0, agent: str = "random", noise: float = 0.1,
                       seat: Optional[torch.Tensor] = None, value_scale: int = 256, out: Optional[dict] = None):
        """``mcts`` with Voronoi territory as the leaf evaluator, ONE launch (``crl_tron_mcts_territory``; boards up to
        64x64): the same tree over the SEAT's three actions, the same model ``agent`` in the tree steps, but a new leaf is
        valued by one flood of its position instead of playouts -- ``floor(2 V a_s / (a_s + a_o))`` half-points on the
        scale V = ``value_scale`` (1 .. 1024), with a_s the seat's territory and a_o the best other live player's; V when
        nobody has any; a closed leaf 2 V if the seat is alive, else 0.  Nothing is drawn at a leaf.  ``simulations`` is at
        most ``mcts_max_simulations``; ``exploration`` as in ``mcts``.  Returns {'visits', 'value' int32 [B, 3], 'nodes',
        'best' int32 [B]} as ``mcts`` does ('value' on the scale of V); ``out`` reuses such a dict.  The state is only read.
        No host synchronisation; capturable into a graph."""
        S = _int_in("simulations", simulations, 1, self.mcts_max_simulations)
        cexp = _exploration("exploration", exploration)
        _one_of("agent", agent, ("random", "avoid"))
        noise = _unit("noise", noise)
        _seat(seat, self.B, self.device)
        V = _int_in("value_scale", value_scale, 1, 1024)
        i32 = torch.int32
        out = _out_dict(out, {"visits": (i32, (self.B, 3)), "value": (i32, (self.B, 3)), "nodes": (i32, (self.B,)),
                              "best": (i32, (self.B,))}, self.device)
        self._call("crl_tron_mcts_territory", _seed(seed), self.first_env_id, *self._state(), _ptr(self.tcount), _ptr(seat), S, V,
                   cexp, noise, _ptr(out["visits"]), _ptr(out["value"]), _ptr(out["nodes"]), _ptr(out["best"]),
                   _native.CRL_PLAYOUT_AVOID if agent == "avoid" else 0)
        return out

    def mcts_territory_action(self, simulations: int, seed: int = 0, exploration: float = 1.0, agent: str = "random",
                              noise: float = 0.1, seat: Optional[torch.Tensor] = None, value_scale: int = 256,
                              out: Optional[dict] = None) -> torch.Tensor:
        """``mcts_territory``'s most visited action as an int64 [B] action for ``step_single`` (-1 where the seat is dead or
        the game is over): the kernel's own ``best``, only widened here.  No host synchronisation; capturable."""
        return self.mcts_territory(simulations, seed, exploration, agent, noise, seat, value_scale, out)["best"].to(torch.int64)

    # -- the search valued by the caller's network (PUCT); the contract is with crl_tron_puct_begin in include/colosseum_hip.h
    PUCT_MAX_CAPACITY = 4095

    def _puct_open(self):
        if getattr(self, "_puct_cap", None) is None:
            raise ValueError("no search is open: call puct_begin(capacity) first")
        return self._puct_tree, self._puct_cap

    def _puct_select_spec(self):
        B, P, NN = self.B, self.P, self.N * self.N
        i8, i16 = torch.int8, torch.int16
        return {"obs_board": (i8, (B, NN)), "obs_heads": (i16, (P, B)), "obs_dirs": (i8, (P, B)), "obs_deaths": (i8, (P, B)),
                "pending": (torch.uint8, (B,)), "depth": (torch.int32, (B,)),
                "leaf_board": (i8, (B, NN)), "leaf_heads": (i16, (P, B)), "leaf_dirs": (i8, (P, B)), "leaf_deaths": (i8, (P, B))}

    def _puct_root_spec(self):
        i32 = torch.int32
        return {"visits": (i32, (self.B, 3)), "value": (i32, (self.B, 3)), "prior": (i32, (self.B, 3)), "nodes": (i32, (self.B,)),
                "sims": (i32, (self.B,)), "best": (i32, (self.B,))}

    def puct_begin(self, capacity: int, seed: int = 0, agent: str = "random", noise: float = 0.1,
                   seat: Optional[torch.Tensor] = None):
        """Opens a search of at most ``capacity`` (1 .. 4095) simulations for the seat ``seat[b]`` (int8 [B]; None: player 0)
        from every game's position (``crl_tron_puct_begin``).  The tree branches on the SEAT's three actions; the other
        players are part of the transition, played by ``agent`` ("random", or "avoid" with ``noise``) from draws keyed by
        ``seed``, the game ids and ``tcount``.  The trees live in a device tensor of this stepper, allocated here or reused
        when the capacity is the last one's, and hold their own copy of the position -- the batch may be stepped while the
        search is open.  A dead seat, a seat out of range and a finished game make skipped trees.  One launch, no host
        synchronisation."""
        cap = _int_in("capacity", capacity, 1, self.PUCT_MAX_CAPACITY)
        _one_of("agent", agent, ("random", "avoid"))
        noise = _unit("noise", noise)
        _seat(seat, self.B, self.device)
        if getattr(self, "_puct_cap", None) != cap:
            nbytes = self._lib.crl_tron_puct_tree_bytes(self._ctx.handle, cap)
            if nbytes < 0:
                check(int(nbytes), "crl_tron_puct_tree_bytes")
            with torch.cuda.device(self.device):
                self._puct_tree = torch.empty((self.B, int(nbytes) // 16, 2), dtype=torch.int64, device=self.device)   # (16-byte units)
            self._puct_cap = cap
        self._call("crl_tron_puct_begin", _seed(seed), self.first_env_id, *self._state(), _ptr(self.tcount), _ptr(seat), cap, noise,
                   _native.CRL_PLAYOUT_AVOID if agent == "avoid" else 0, _ptr(self._puct_tree))

    def puct_select(self, exploration: float = 1.25, fpu: float = 0.5, out: Optional[dict] = None):
        """One descent of every open tree (``crl_tron_puct_select``): ``exploration`` is c of the PUCT score (0 .. 65535 / 256),
        ``fpu`` the value in [0, 1] of a child without a visit.  Returns the leaves that wait for the caller's network:
        {'obs_board' int8 [B, N*N], 'obs_heads' int16 [P, B], 'obs_dirs', 'obs_deaths' int8 [P, B]: the leaf as ``observe``
        shows it to the seat, 'pending' uint8 [B], 'depth' int32 [B]: the edges from the root (the leaf's counter base is
        tcount + depth), 'leaf_board', 'leaf_heads', 'leaf_dirs', 'leaf_deaths': the leaf position in the state layout, for
        ``territory`` or ``playout`` of another stepper}; rows whose tree has no pending leaf (skipped, a terminal leaf, at
        capacity) are zeros.  ``out`` reuses such a dict.  One launch, no host synchronisation."""
        tree, cap = self._puct_open()
        cpuct = _exploration("exploration", exploration)
        fpu16 = int(round(65536.0 * _unit("fpu", fpu)))
        out = _out_dict(out, self._puct_select_spec(), self.device)
        self._call("crl_tron_puct_select", _ptr(tree), cap, cpuct, fpu16, _ptr(out["obs_board"]), _ptr(out["obs_heads"]),
                   _ptr(out["obs_dirs"]), _ptr(out["obs_deaths"]), _ptr(out["pending"]), _ptr(out["depth"]), _ptr(out["leaf_board"]),
                   _ptr(out["leaf_heads"]), _ptr(out["leaf_dirs"]), _ptr(out["leaf_deaths"]), 0)
        return out

    def puct_backup(self, prior: torch.Tensor, value: torch.Tensor):
        """Expands the pending leaves with ``prior`` (uint16 [B, 3], or int16 of the same bits: any weights for forward, right,
        left, normalised by the backup) and backs ``value`` up (int32 [B]: the seat's value on 0 .. 65536); terminal leaves
        back their outcome up (``crl_tron_puct_backup``).  One launch."""
        tree, cap = self._puct_open()
        if not isinstance(prior, torch.Tensor) or prior.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
            raise ValueError("prior must be a uint16 (or int16) tensor of shape (%d, 3)" % self.B)
        _want(prior, prior.dtype, (self.B, 3), self.device, "prior")
        if not isinstance(value, torch.Tensor):
            raise ValueError("value must be an int32 tensor of shape (%d,)" % self.B)
        _want(value, torch.int32, (self.B,), self.device, "value")
        self._call("crl_tron_puct_backup", _ptr(tree), cap, _ptr(prior), _ptr(value), 0)

    def puct_root(self, out: Optional[dict] = None):
        """The root of every open tree (``crl_tron_puct_root``): {'visits', 'value', 'prior' int32 [B, 3]: simulations through
        the root's child at each action (0 forward, 1 right, 2 left), the seat's summed value there (65536 per won simulation)
        and the root's stored priors, 'nodes', 'sims', 'best' int32 [B]: the most visited action (ties: the larger value, then
        the lower action; -1 without a visited child)}.  The visit counts are the policy target of an AlphaZero-style trainer.
        One launch."""
        tree, cap = self._puct_open()
        out = _out_dict(out, self._puct_root_spec(), self.device)
        self._call("crl_tron_puct_root", _ptr(tree), cap, _ptr(out["visits"]), _ptr(out["value"]), _ptr(out["prior"]),
                   _ptr(out["nodes"]), _ptr(out["sims"]), _ptr(out["best"]))
        return out

    @staticmethod
    def puct_quantize(policy: torch.Tensor, value: torch.Tensor):
        """(float policy [B, 3]: any non-negative weights, float value [B] in [0, 1]) -> (int16 prior holding the contract's
        uint16 bits, int32 value on 0 .. 65536) for ``puct_backup``.  Each row's weights are scaled so that its greatest is
        65535 (the backup normalises anyway); NaN counts as 0 in the policy and as 0.5 in the value.  Torch operations only."""
        pol = torch.nan_to_num(policy.to(torch.float32), nan=0.0, posinf=0.0).clamp_min(0.0)
        top = pol.amax(dim=1, keepdim=True).clamp_min(1e-30)
        q = torch.round(pol * (65535.0 / top)).to(torch.int32).clamp(0, 65535)
        prior = torch.where(q >= 32768, q - 65536, q).to(torch.int16)
        val = torch.round(torch.nan_to_num(value.to(torch.float32), nan=0.5).clamp(0.0, 1.0) * 65536.0).to(torch.int32)
        return prior.contiguous(), val.contiguous()

    def puct(self, evaluate, simulations: int, exploration: float = 1.25, fpu: float = 0.5, seed: int = 0, agent: str = "random",
             noise: float = 0.1, seat: Optional[torch.Tensor] = None, out: Optional[dict] = None):
        """A whole search: ``puct_begin(simulations, seed, agent, noise, seat)``, then ``simulations`` times ``puct_select`` ->
        ``evaluate(leaves)`` -> ``puct_backup``, then ``puct_root``.  ``evaluate`` takes the select dict and returns (prior,
        value), either the integer tensors of ``puct_backup`` or float tensors (then ``puct_quantize`` turns them).  Two
        launches per simulation beside the caller's network; no host synchronisation.  Returns the root dict (``out`` reuses
        one)."""
        if not callable(evaluate):
            raise ValueError("evaluate must be callable: the select dict -> (prior, value)")
        S = _int_in("simulations", simulations, 1, self.PUCT_MAX_CAPACITY)
        _exploration("exploration", exploration), _unit("fpu", fpu)
        self.puct_begin(S, seed, agent, noise, seat)
        leaves = None
        for _ in range(S):
            leaves = self.puct_select(exploration, fpu, out=leaves)
            prior, value = evaluate(leaves)
            if prior.is_floating_point() or value.is_floating_point():
                prior, value = self.puct_quantize(prior, value)
            self.puct_backup(prior, value)
        return self.puct_root(out)

    def puct_action(self, evaluate, simulations: int, exploration: float = 1.25, fpu: float = 0.5, seed: int = 0,
                    agent: str = "random", noise: float = 0.1, seat: Optional[torch.Tensor] = None,
                    out: Optional[dict] = None) -> torch.Tensor:
        """``puct``'s most visited action as an int64 [B] action in {0, 1, 2} for ``step_single`` (-1 where the seat is dead or
        the game is over)."""
        return self.puct(evaluate, simulations, exploration, fpu, seed, agent, noise, seat, out)["best"].to(torch.int64)

    # -- Voronoi territory of every game's position (the deterministic evaluator beside playout)
    def territory(self, candidates: Optional[torch.Tensor] = None, seat: Optional[torch.Tensor] = None,
                  out: Optional[dict] = None):
        """Voronoi territory from every game's position, ONE launch (``crl_tron_territory``): ``area[b, a, p]`` is the
        number of free cells player p reaches strictly before every other live player when the seat ``seat[b]`` (int8 [B];
        None: player 0) first plays ``candidates[b, a]`` (int32 [B, A], A <= 16: 0 forward, 1 right, 2 left; any other
        value skips the row).  ``candidates=None`` evaluates the position as it stands (A = 1, nobody forced).  Returns
        {'area' int32 [B, A, P], 'info' uint8 [B, A]} -- info bit 0: the row was evaluated, bit 1: the forced cell is off
        the board or occupied; skipped rows are zeros; ``out`` reuses such a dict.  The state is only read.  No host
        synchronisation; capturable into a graph."""
        _seat(seat, self.B, self.device)
        A = _candidates(candidates, self.B, self.device, 16)
        out = _out_dict(out, {"area": (torch.int32, (self.B, A, self.P)), "info": (torch.uint8, (self.B, A))}, self.device)
        self._call("crl_tron_territory", *self._state(), _ptr(seat), _ptr(candidates), A, _ptr(out["area"]), _ptr(out["info"]))
        return out

    def territory_action(self, seat: Optional[torch.Tensor] = None, out: Optional[dict] = None) -> torch.Tensor:
        """The territory-greedy action for the seat in every game: ``territory`` on the three first actions [0, 1, 2],
        score = the seat's area minus the best other live player's (a fatal action below every other), the best action
        (ties: the lowest) as int64 [B] in {0, 1, 2} for ``step_single`` -- the noise-free rule of ``sample_territory``;
        -1 where every row was skipped (the seat is dead).  ``out``: the territory dict to reuse.  No host
        synchronisation; capturable."""
        o = self.territory(self._moves3, seat, out)
        area = o["area"].to(torch.int64)                                          # [B, 3, P]
        who = (torch.zeros((self.B,), dtype=torch.int64, device=self.device) if seat is None else seat.to(torch.int64))
        who = who.clamp(0, self.P - 1).view(self.B, 1, 1).expand(self.B, 3, 1)
        own = torch.gather(area, 2, who).squeeze(2)
        others = (self.deaths.t() == 0).view(self.B, 1, self.P).expand(self.B, 3, self.P).clone()
        others.scatter_(2, who, False)
        rival = torch.where(others, area, torch.zeros_like(area)).amax(dim=2)     # (no other live player: 0)
        score = torch.where((o["info"] & 2) != 0, torch.full_like(own, -(1 << 30)), own - rival)
        score = torch.where((o["info"] & 1) != 0, score, torch.full_like(score, -(1 << 31)))
        best = torch.argmax(score, dim=1)                                         # (the first of equal maxima)
        return torch.where((o["info"] & 1).amax(dim=1) != 0, best, torch.full_like(best, -1))

    # -- the territory-greedy scripted opponent for one step: int8 [P][B] actions in the step() encoding
    def sample_territory(self, seed: int = 0, noise: float = 0.1, players=None, out: Optional[torch.Tensor] = None,
                         advance: bool = True):
        """Actions of the territory-greedy agent at each game's step counter (``tcount``), under the contract of
        ``crl_tron_sample_territory`` (include/colosseum_hip.h): with probability ``noise`` a uniform action, else the
        first action with the best Voronoi score (own area minus the best rival's), decided on the current (pre-step)
        boards.  ``players`` / ``out`` / ``advance`` as ``sample_avoid``: only the named players' rows of ``out`` (int8
        [P, B]; a new zeroed tensor when None) are written."""
        _unit("noise", noise)          # (ValueError here; sample_avoid leaves a bad noise to its C entry: NativeError)
        return self._sample_scripted("sample_territory", seed, noise, players, out, advance)

    # -- the territory tree search as a seated opponent for one step; the contract is with crl_tron_sample_mcts_territory
    def mcts_agent_max_simulations(self, players=None) -> int:
        """the most simulations ``sample_mcts_territory`` takes for these ``players`` (None: all) on this board
        (``crl_tron_sample_mcts_territory_max_simulations``: the trees of a game's players share one workgroup's LDS, so
        the more players search, the smaller each tree); boards wider than 64 have no such agent and raise here"""
        mask = _player_mask(players, self.P, "mcts_agent_max_simulations")
        if mask == 0:
            raise ValueError("mcts_agent_max_simulations: players is empty")
        rc = self._lib.crl_tron_sample_mcts_territory_max_simulations(self._ctx.handle, mask)
        if rc < 0:
            check(rc, "crl_tron_sample_mcts_territory_max_simulations")
        return int(rc)

    def sample_mcts_territory(self, simulations: int, seed: int = 0, exploration: float = 1.0, noise: float = 0.0, players=None,
                              out: Optional[torch.Tensor] = None, advance: bool = True, agent: str = "random",
                              model_noise: float = 0.1, value_scale: int = 256):
        """Actions of the territory tree search seated at ``players`` at each game's step counter (``tcount``), ONE launch
        (``crl_tron_sample_mcts_territory``; boards up to 64x64): with probability ``noise`` a uniform action (the draw of
        ``sample_territory``), else the ``best`` of ``mcts_territory(simulations, seed, exploration, agent, model_noise,
        seat=p, value_scale)`` for each named player p, all decided on the current (pre-step) boards; a player in a game
        that is over plays 0.  ``simulations`` is at most ``mcts_agent_max_simulations(players)``.  ``players`` / ``out`` /
        ``advance`` as ``sample_avoid``: only the named players' rows of ``out`` (int8 [P, B] in the ``step`` encoding; a new
        zeroed tensor when None) are written, and the counter advances once per game.  No host synchronisation; capturable
        into a graph."""
        mask = _player_mask(players, self.P, "sample_mcts_territory")
        if mask == 0:
            raise ValueError("sample_mcts_territory: players is empty")
        cexp = _exploration("exploration", exploration)
        noise = _unit("noise", noise)
        _one_of("agent", agent, ("random", "avoid"))
        model_noise = _unit("model_noise", model_noise)
        V = _int_in("value_scale", value_scale, 1, 1024)
        S = _int_in("simulations", simulations, 1, self.mcts_agent_max_simulations(players))
        if out is None:
            out = torch.zeros((self.P, self.B), dtype=torch.int8, device=self.device)
        else:
            _want(out, torch.int8, (self.P, self.B), self.device, "out")
        self._call("crl_tron_sample_mcts_territory", _seed(seed), self.first_env_id, _ptr(self.tcount), int(advance), noise, mask,
                   *self._state(), S, V, cexp, model_noise, _native.CRL_PLAYOUT_AVOID if agent == "avoid" else 0, _ptr(out))
        return out

    # -- T fused steps with every player on the avoid agent, auto-reset
    def rollout_avoid(self, steps: int, seed: int = 0, noise: float = 0.1):
        """``rollout`` with every player on the reference's ``SimpleAvoidAgent(noise)`` instead of the random agent
        (``crl_tron_rollout_avoid``): the same statistics tensors, ``results()`` rows and step counter."""
        steps = int(steps)
        self._call("crl_tron_rollout_avoid", _seed(seed), self.first_env_id, steps, float(noise),
                   *(self._rollout_args or self._bind_rollout()), 0)
        self._stat_steps += steps

    # -- state_to_observation for all games; player int8 [B]
    def observe(self, player: torch.Tensor):
        _want(player, torch.int8, (self.B,), self.device, "player")
        ob = torch.empty_like(self.board)
        oh = torch.empty_like(self.heads)
        od = torch.empty_like(self.dirs)
        ok = torch.empty_like(self.deaths)
        self._call("crl_tron_observe", *self._state(), _ptr(player), _ptr(ob), _ptr(oh), _ptr(od), _ptr(ok))
        return {"board": ob.view(self.B, self.N, self.N), "heads": oh, "directions": od, "deaths": ok}

    # -- state_to_observation of every game for every observer in one pass
    def observe_all(self, out: Optional[dict] = None):
        """{'board': int8 [P, B, N, N], 'heads': int16 [P, P, B], 'directions' / 'deaths': int8 [P, P, B]};
        slice [p] is what player p observes.  Pass a previous result as `out` to reuse its buffers."""
        out = out or self.observe_all_buffers()
        self._call("crl_tron_observe_all", *self._state(), _ptr(out["board"]), _ptr(out["heads"]), _ptr(out["directions"]),
                   _ptr(out["deaths"]))
        return out

    # -- [sample ->] next_state -> state_to_observation of all observers, one launch
    def step_observe(self, actions: Optional[torch.Tensor] = None, seed: int = 0, auto_reset: bool = True,
                     out: Optional[dict] = None):
        """What a self-play learner needs every step, fused: plays `actions` (int8 [P, B]; None = the rollout's random
        agent at each game's step counter, which then advances) and returns the observations of ALL P players of the
        resulting states together with the step outputs:
        {'board' [P, B, N, N], 'heads' [P, P, B], 'directions', 'deaths', 'rewards' [P, B], 'terminal' [B], 'winners' [B]}.
        Equals ``step(sample(seed) or actions, auto_reset); observe_all()``; one launch on every board size and player
        count.  Pass a previous result as `out` to reuse its observation buffers."""
        if actions is not None:
            _want(actions, torch.int8, (self.P, self.B), self.device, "actions")
        out = out or self.observe_all_buffers()
        self._call("crl_tron_step_observe", _seed(seed), self.first_env_id, *self._state(), _ptr(actions), _ptr(self.tcount),
                   _ptr(self.rewards), _ptr(self.terminal), _ptr(self.winners), _ptr(out["board"]), _ptr(out["heads"]),
                   _ptr(out["directions"]), _ptr(out["deaths"]), CRL_STEP_AUTO_RESET if auto_reset else 0)
        out["rewards"], out["terminal"], out["winners"] = self.rewards, self.terminal, self.winners
        return out

    def observe_all_buffers(self):
        P, B, N = self.P, self.B, self.N
        return _alloc({"board": (torch.int8, (P, B, N, N)), "heads": (torch.int16, (P, P, B)),
                       "directions": (torch.int8, (P, P, B)), "deaths": (torch.int8, (P, P, B))}, self.device)

    # -- the learner's action index + the opponents' actions -> next_state, done, reset of done games, one launch
    def step_single(self, actions: torch.Tensor, learner_action: torch.Tensor, reward: torch.Tensor, done: torch.Tensor,
                    terminal: torch.Tensor):
        """One step of "learner = player 0 against scripted opponents" in every game (``crl_tron_step_single``): player 0
        plays ``learner_action`` (int64 [B]: 0 forward, 1 right, 2 left), the others their rows of ``actions`` (int8 [P, B] in
        the ``step`` encoding, e.g. filled by ``sample_avoid(players=...)``; row 0 is ignored); games that are done
        restart.  Writes the caller's ``reward`` int8 [B] (the learner's), ``done`` uint8 [B] (learner dead or game over)
        and ``terminal`` uint8 [B] (the game itself ended).  No host synchronisation; capturable into a graph."""
        _want(actions, torch.int8, (self.P, self.B), self.device, "actions")
        _want(learner_action, torch.int64, (self.B,), self.device, "learner_action")
        _want(reward, torch.int8, (self.B,), self.device, "reward")
        _want(done, torch.uint8, (self.B,), self.device, "done")
        _want(terminal, torch.uint8, (self.B,), self.device, "terminal")
        self._call("crl_tron_step_single", *self._state(), _ptr(actions), _ptr(learner_action), _ptr(reward), _ptr(done),
                   _ptr(terminal))

    # -- compute_ranking for all games: int8 [P, B], 0 = best
    def ranking(self):
        out = torch.empty((self.P, self.B), dtype=torch.int8, device=self.device)
        self._call("crl_tron_ranking", _ptr(self.board), _ptr(self.deaths), _ptr(out))
        return out

    def results(self, copy: bool = True):
        """Per-game episode results packed for the end-of-rollout gather: int32 [B, 3+2P] =
        n_episodes, len_sum, last_winners, win_count[P], ret_sum[P].  The rows are written by the rollout kernel
        itself at the end of every launch (``crl_tron_stats.results``): no packing pass.  By default a snapshot;
        ``copy=False`` hands out the live buffer, which the next rollout rewrites in place."""
        return self._results.clone() if copy else self._results

    rollout_takes_events = True    # rollout(events=(start, stop)): HIP events attached to the dispatches

    PACKED_EXACT_STEPS = 3276      # |ret_sum| <= 10 per step: the int16 fields hold the totals of this many steps

    def packed_rows_exact(self) -> bool:
        """True while the 16-bit row of ``results_packed`` cannot have wrapped: the running totals span at most
        ``PACKED_EXACT_STEPS`` rollout steps since ``reset_stats`` (known on the host: it issues the launches)."""
        return self._stat_steps <= self.PACKED_EXACT_STEPS

    def results_packed(self, copy: bool = True):
        """The gather row in 16-bit fields: int16 [B, (4+P+1)&~1] = n_episodes, len_sum, last_winners, tstep (steps into
        the unfinished episode), ret_sum[P] -- the low 16 bits of the running totals, written by the rollout kernel
        (``crl_tron_stats.packed``); 16 bytes per game at P = 4 instead of 44.  Exact while ``packed_rows_exact()``."""
        return self._packed.clone() if copy else self._packed

    def results_from_columns(self):
        """The same rows assembled from the per-column statistics (what ``results()`` must equal; used by the tests)."""
        cols = [self.n_episodes, self.len_sum, self.last_winners.to(torch.int32)]
        cols += [self.win_count[p] for p in range(self.P)] + [self.ret_sum[p] for p in range(self.P)]
        return torch.stack(cols, dim=1).contiguous()

    def results_packed_from_columns(self):
        """The 16-bit rows assembled from the per-column statistics (what ``results_packed()`` must equal; tests)."""
        cols = [self.n_episodes, self.len_sum, self.last_winners.to(torch.int32), self.tstep]
        cols += [self.ret_sum[p] for p in range(self.P)]
        cols += [torch.zeros_like(self.tstep)] * (self._packed.shape[1] - len(cols))
        return torch.stack(cols, dim=1).to(torch.int16).contiguous()


class TTTBatch(_RolloutStepper):
    """B games of n-player TicTacToe on a dims board, K in a row (reference: envs/tictactoe/*).

    State tensors (device): occ int32 [P, B] bit masks; winner int8 [B] (-1 none); to_move int8 [B].
    """

    STATS_STRUCT = _native.TTTStats
    PLAN_BIND = "crl_ttt_rollout_bind"
    STATS = {"tcount": (torch.int32, _per_game), "tstep": (torch.int32, _per_game), "n_episodes": (torch.int32, _per_game),
             "win_count": (torch.int32, _per_player), "draw_count": (torch.int32, _per_game), "len_sum": (torch.int32, _per_game),
             "results": (torch.int32, lambda B, P: (B, 3 + P))}

    def __init__(self, dims: Sequence[int] = (3, 3), k: int = 3, num_players: int = 2, batch: int = 1,
                 device="cuda", first_env_id: int = 0):
        self.dims = tuple(int(d) for d in dims)
        d3 = (1,) * (3 - len(self.dims)) + self.dims
        self.K, self.P, self.B = int(k), int(num_players), int(batch)
        self.n_cells = d3[0] * d3[1] * d3[2]
        self._open(device, first_env_id, "crl_ttt_create", d3[0], d3[1], d3[2], self.K, self.P)
        dev, B, P = self.device, self.B, self.P
        with torch.cuda.device(dev):
            self.occ = torch.zeros((P, B), dtype=torch.int32, device=dev)
            self.winner = torch.full((B,), -1, dtype=torch.int8, device=dev)
            self.to_move = torch.zeros((B,), dtype=torch.int8, device=dev)
            self.reward = torch.zeros((B,), dtype=torch.int8, device=dev)
            self.terminal = torch.zeros((B,), dtype=torch.uint8, device=dev)
            self.winners = torch.zeros((B,), dtype=torch.int8, device=dev)
            self.__dict__.update(_alloc(self._stat_spec(B, P), dev, torch.zeros))
        self._open_wait()

    def _state(self):
        return (_ptr(self.occ), _ptr(self.winner), _ptr(self.to_move))

    def lines(self):
        buf = (C.c_uint32 * 256)()
        n = self._lib.crl_ttt_lines(self._ctx.handle, buf, 256)
        return [int(buf[i]) for i in range(n)]

    def reset(self, mask: Optional[torch.Tensor] = None):
        if mask is not None:
            _want(mask, torch.uint8, (self.B,), self.device, "mask")
        self._call("crl_ttt_reset", _ptr(mask), _ptr(self.occ), _ptr(self.winner), _ptr(self.to_move))

    def step(self, action: torch.Tensor, auto_reset: bool = False):
        _want(action, torch.int8, (self.B,), self.device, "action")
        self._call("crl_ttt_step", _ptr(self.occ), _ptr(self.winner), _ptr(self.to_move), _ptr(action), _ptr(self.reward),
                   _ptr(self.terminal), _ptr(self.winners), CRL_STEP_AUTO_RESET if auto_reset else 0)
        return self.reward, self.terminal, self.winners

    def valid_mask(self):
        out = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        self._call("crl_ttt_valid", _ptr(self.occ), _ptr(out))
        return out

    def sample(self, seed: int = 0, advance: bool = True):
        """The rollout's random agent for one step: int8 [B] flat cell (uniform over the empty cells, -1 on a full
        board) at each game's step counter; ``step(sample(seed), auto_reset=True)`` T times == ``rollout(T, seed)``."""
        act = torch.empty((self.B,), dtype=torch.int8, device=self.device)
        self._call("crl_ttt_sample", _seed(seed), self.first_env_id, _ptr(self.occ), _ptr(self.tcount), int(advance), _ptr(act))
        return act

    # -- the tactical (win-or-block) agent; the contract is with crl_ttt_sample_tactical in include/colosseum_hip.h
    AGENTS = ("random", "tactical")

    def winning_cells(self):
        """int32 [P, B]: per player the mask of empty cells that complete a K-line for it (``crl_ttt_winning_cells``) -- an
        observation feature / action prior, and the set the tactical agent plays from."""
        out = torch.empty((self.P, self.B), dtype=torch.int32, device=self.device)
        self._call("crl_ttt_winning_cells", _ptr(self.occ), _ptr(out))
        return out

    def sample_tactical(self, seed: int = 0, noise: float = 0.1, advance: bool = True):
        """The tactical agent for one step: int8 [B] flat cell at each game's step counter -- with probability ``noise`` a
        uniform empty cell, else a winning cell of the mover if it has one, else a cell that blocks the earliest upcoming
        player who has one, else a uniform empty cell; -1 on a full board.
        ``step(sample_tactical(seed, noise), auto_reset=True)`` T times == ``rollout_tactical(T, seed, noise)``."""
        noise = _unit("noise", noise)
        act = torch.empty((self.B,), dtype=torch.int8, device=self.device)
        self._call("crl_ttt_sample_tactical", _seed(seed), self.first_env_id, _ptr(self.occ), _ptr(self.to_move),
                   _ptr(self.tcount), int(advance), noise, _ptr(act))
        return act

    def rollout_tactical(self, steps: int, seed: int = 0, noise: float = 0.1):
        """``rollout`` with every seat on the tactical agent (``crl_ttt_rollout_tactical``): the same statistics tensors,
        ``results()`` rows and step counter."""
        noise = _unit("noise", noise)
        self._call("crl_ttt_rollout_tactical", _seed(seed), self.first_env_id, int(steps), noise, _ptr(self.occ),
                   _ptr(self.winner), _ptr(self.to_move), self._stats())

    def board(self, player: Optional[torch.Tensor] = None, rel_mod: Optional[int] = None):
        out = torch.empty((self.B, self.n_cells), dtype=torch.int8, device=self.device)
        if player is not None:
            _want(player, torch.int8, (self.B,), self.device, "player")
        self._call("crl_ttt_board", _ptr(self.occ), _ptr(player), int(rel_mod if rel_mod else self.P), _ptr(out))
        return out

    def observe(self, player: torch.Tensor, rel_mod: Optional[int] = None):
        """state_to_observation for all games: board with ids relative to player[b] (reference 2p:382-407)."""
        return {"board": self.board(player, rel_mod)}

    def _obs_spec(self):
        """the buffers `step_observe` and `step_single` fill for the next mover / the learner"""
        return {"board": (torch.int8, (self.B, self.n_cells)), "valid": (torch.int32, (self.B,))}

    def step_observe(self, action: Optional[torch.Tensor] = None, seed: int = 0, auto_reset: bool = True,
                     rel_mod: Optional[int] = None, out: Optional[dict] = None):
        """One ply of every game in ONE launch: plays `action` (int8 [B]; None = the rollout's random agent at each
        game's step counter, which then advances) and returns what the next mover needs:
        {'board' int8 [B, cells] relative to the player to move next, 'valid' int32 [B] empties mask, 'mover' int8 [B],
        'reward', 'terminal', 'winners'}.  Equals ``step(...); valid_mask(); board(to_move, rel_mod)``."""
        if action is not None:
            _want(action, torch.int8, (self.B,), self.device, "action")
        out = out or _alloc(self._obs_spec(), self.device)
        self._call("crl_ttt_step_observe", _seed(seed), self.first_env_id, _ptr(self.occ), _ptr(self.winner), _ptr(self.to_move),
                   _ptr(action), _ptr(self.tcount), _ptr(self.reward), _ptr(self.terminal), _ptr(self.winners),
                   _ptr(out["board"]), _ptr(out["valid"]), int(rel_mod if rel_mod else self.P),
                   CRL_STEP_AUTO_RESET if auto_reset else 0)
        out["mover"], out["reward"], out["terminal"], out["winners"] = self.to_move, self.reward, self.terminal, self.winners
        return out

    def step_single(self, seat: torch.Tensor, learner_action: Optional[torch.Tensor] = None, seed: int = 0,
                    rel_mod: Optional[int] = None, out: Optional[dict] = None, opponent: str = "random", noise: float = 0.1,
                    simulations: Optional[int] = None, playouts: int = 16, exploration: float = 1.0):
        """One step of "learner at seat[b] against the random agent" in every game, ONE launch (``crl_ttt_step_single``):
        the learner plays ``learner_action`` (int64 [B]: a cell in [-1, cells), anything else passes) when it is its turn,
        the random agent plays every other seat until it is the learner's turn again, finished games restart on the way.
        ``learner_action=None`` only advances to the learner's turn.  seat int8 [B].  Returns
        {'board' int8 [B, cells] relative to the learner, 'valid' int32 [B] empties mask, 'reward' int8 [B] (+1 the learner
        won, -1 another player, 0 draw or not over), 'done' uint8 [B], 'winners' int8 [B]}; every ply, the learner's
        included, advances ``tcount`` (the draws are ``sample``'s).  ``opponent="tactical"``: every other seat plays the
        tactical agent with ``noise`` instead (``crl_ttt_step_single_tactical``; the draws are ``sample_tactical``'s).
        ``opponent="mcts"``: every other seat plays the search agent (``crl_ttt_step_single_mcts``; ``sample_mcts``'s moves) with
        ``simulations`` (required), ``playouts``, ``exploration`` and ``noise``; still one launch."""
        _want(seat, torch.int8, (self.B,), self.device, "seat")
        if learner_action is not None:
            _want(learner_action, torch.int64, (self.B,), self.device, "learner_action")
        opponent = _one_of("opponent", opponent, self.OPPONENTS)
        noise = _unit("noise", noise)
        if opponent == "mcts":
            if simulations is None:
                raise ValueError("opponent='mcts' needs simulations")
            name, tail = "crl_ttt_step_single_mcts", self._search_args(simulations, playouts, exploration) + (noise, 0)
        else:
            name, tail = ("crl_ttt_step_single_tactical", (noise, 0)) if opponent == "tactical" else ("crl_ttt_step_single", (0,))
        out = out or _alloc(dict(self._obs_spec(), done=(torch.uint8, (self.B,))), self.device)
        self._call(name, _seed(seed), self.first_env_id,
                   _ptr(self.occ), _ptr(self.winner), _ptr(self.to_move), _ptr(seat), _ptr(learner_action), _ptr(self.tcount),
                   _ptr(self.reward), _ptr(out["done"]), _ptr(self.winners), _ptr(out["board"]), _ptr(out["valid"]),
                   int(rel_mod if rel_mod else self.P), *tail)
        out["reward"], out["winners"] = self.reward, self.winners
        return out

    def playout(self, playouts: int, candidates: Optional[torch.Tensor] = None, seed: int = 0, out: Optional[dict] = None,
                agent: str = "random", noise: float = 0.1):
        """Random playouts from every game's position, ONE launch (``crl_ttt_playout``): row (b, a) plays candidate cell
        ``candidates[b, a]`` (int32 [B, A]; an occupied cell, -1 or a value outside [0, cells) skips the row) for the
        player to move and then ``playouts`` random games to their end, on private copies; ``candidates=None`` evaluates
        the position as it stands (A = 1).  Finished positions skip every row.  The draws are keyed by ``seed``, the game
        ids and ``tcount`` as the counter base (which the call neither advances nor writes; the state is only read).
        Returns {'wins' int32 [B, A, P], 'draws', 'played', 'len_sum' int32 [B, A]} (skipped rows are zeros); ``out``
        reuses such a dict.  ``agent="tactical"``: every ply after the candidate is the tactical agent's with ``noise``
        (``crl_ttt_playout_tactical``, draws under a tag of their own).  No host synchronisation; capturable into a graph."""
        R = _int_in("playouts", playouts, 1, 65535)
        A = _candidates(candidates, self.B, self.device, 65535)
        tactical = _one_of("agent", agent, self.AGENTS) == "tactical"
        noise = _unit("noise", noise)
        i32, BA = torch.int32, (self.B, A)
        out = _out_dict(out, {"wins": (i32, BA + (self.P,)), "draws": (i32, BA), "played": (i32, BA), "len_sum": (i32, BA)},
                        self.device)
        self._call("crl_ttt_playout_tactical" if tactical else "crl_ttt_playout", _seed(seed), self.first_env_id, _ptr(self.occ),
                   _ptr(self.winner), _ptr(self.to_move), _ptr(self.tcount), _ptr(candidates), A, R, _ptr(out["wins"]),
                   _ptr(out["played"]), _ptr(out["len_sum"]), *((noise, 0) if tactical else (0,)))
        torch.sub(out["played"], out["wins"].sum(dim=2, dtype=torch.int32), out=out["draws"])
        return out

    @functools.cached_property
    def _all_cells(self):
        """int32 [B, cells]: every cell of every game, `flat_mc_action`'s candidates (made at the first use)"""
        return torch.arange(self.n_cells, dtype=torch.int32, device=self.device).expand(self.B, self.n_cells).contiguous()

    def flat_mc_action(self, playouts: int, seed: int = 0, out: Optional[dict] = None, agent: str = "random",
                       noise: float = 0.1) -> torch.Tensor:
        """Flat Monte Carlo for the player to move in every game: ``playout`` on every cell, value 2 * wins + draws of
        the mover, the best cell (ties: the lowest) as an int64 [B] action for ``step_single``; -1 where no cell could be
        played (the game is over).  ``out``: the playout dict to reuse; ``agent`` / ``noise``: the playout policy, as
        ``playout``.  No host synchronisation; capturable."""
        cells = self._all_cells
        o = self.playout(playouts, cells, seed, out, agent, noise)
        mover = self.to_move.to(torch.int64).clamp(0, self.P - 1)       # (other values: the position skips every row)
        mine = torch.gather(o["wins"], 2, mover.view(-1, 1, 1).expand(self.B, self.n_cells, 1)).squeeze(2)
        return _flat_mc_pick(2 * mine + o["draws"], o["played"], cells)

    # -- Monte Carlo tree search; the contract is with crl_ttt_mcts in include/colosseum_hip.h
    @functools.cached_property
    def mcts_max_simulations(self) -> int:
        """the most simulations ``mcts`` takes on this board (``crl_ttt_mcts_max_simulations``: the tree stays in LDS)"""
        rc = self._lib.crl_ttt_mcts_max_simulations(self._ctx.handle)
        if rc < 0:
            check(rc, "crl_ttt_mcts_max_simulations")
        return int(rc)

    def mcts(self, simulations: int, playouts: int = 16, seed: int = 0, exploration: float = 1.0, out: Optional[dict] = None):
        """A tree search (UCT) for the player to move in every game, ONE launch (``crl_ttt_mcts``): each game builds a tree
        of its own by ``simulations`` descents (at most ``mcts_max_simulations``), each new leaf valued by ``playouts`` (1 ..
        1024) random games to their end; ``exploration`` (0 .. 65535 / 256; 0 = pure exploitation) multiplies
        sqrt(log2 n_parent / n_child) on a value scale of 0 .. 1.  Finished positions are skipped.  The draws are keyed by
        ``seed``, the game ids and ``tcount`` as the counter base (the call reads the state and writes none of it).
        Returns {'visits', 'value' int32 [B, cells]: simulations through the root's child at each cell and its half-points
        (2 per won playout, 1 per drawn one) for the mover, 'nodes' int32 [B], 'best' int32 [B]: the most visited cell (ties:
        the larger value, then the lowest cell; -1 for a skipped position)}; ``out`` reuses such a dict.  The visit counts
        are the policy target of an AlphaZero-style trainer.  No host synchronisation; capturable into a graph."""
        S, R, cexp = self._search_args(simulations, playouts, exploration)
        i32 = torch.int32
        out = _out_dict(out, {"visits": (i32, (self.B, self.n_cells)), "value": (i32, (self.B, self.n_cells)),
                              "nodes": (i32, (self.B,)), "best": (i32, (self.B,))}, self.device)
        self._call("crl_ttt_mcts", _seed(seed), self.first_env_id, _ptr(self.occ), _ptr(self.winner), _ptr(self.to_move),
                   _ptr(self.tcount), S, R, cexp, _ptr(out["visits"]), _ptr(out["value"]), _ptr(out["nodes"]), _ptr(out["best"]), 0)
        return out

    def _search_args(self, simulations, playouts, exploration):
        """(S, R, cexp) of a search as the C entries take them, checked"""
        return (_int_in("simulations", simulations, 1, self.mcts_max_simulations), _int_in("playouts", playouts, 1, 1024),
                _exploration("exploration", exploration))

    def mcts_action(self, simulations: int, playouts: int = 16, seed: int = 0, exploration: float = 1.0,
                    out: Optional[dict] = None) -> torch.Tensor:
        """``mcts``'s most visited cell as an int64 [B] action for ``step_single`` (-1 where the game is over): the arg-max
        is the kernel's own ``best``, only widened here.  No host synchronisation; capturable."""
        return self.mcts(simulations, playouts, seed, exploration, out)["best"].to(torch.int64)

    # -- the search as a seated agent; the contract is with crl_ttt_sample_mcts in include/colosseum_hip.h
    OPPONENTS = AGENTS + ("mcts",)          # who `step_single` seats (`playout` takes AGENTS only)

    def sample_mcts(self, simulations: int, playouts: int = 16, seed: int = 0, exploration: float = 1.0, noise: float = 0.0,
                    advance: bool = True):
        """The search agent for one step (``crl_ttt_sample_mcts``): int8 [B] flat cell at each game's step counter -- with
        probability ``noise`` a uniform empty cell (``sample_tactical``'s draw: at ``noise=1`` the same move), else ``best`` of
        ``mcts(simulations, playouts, seed, exploration)`` on the position with the counter as its base; -1 on a full board.
        ``step(sample_mcts(...), auto_reset=True)`` T times == ``rollout_mcts(T, ...)``.  One launch, a wave per game; no host
        synchronisation, capturable into a graph."""
        S, R, cexp = self._search_args(simulations, playouts, exploration)
        noise = _unit("noise", noise)
        act = torch.empty((self.B,), dtype=torch.int8, device=self.device)
        self._call("crl_ttt_sample_mcts", _seed(seed), self.first_env_id, _ptr(self.occ), _ptr(self.to_move), _ptr(self.tcount),
                   int(advance), S, R, cexp, noise, _ptr(act))
        return act

    def rollout_mcts(self, steps: int, simulations: int, playouts: int = 16, seed: int = 0, exploration: float = 1.0,
                     noise: float = 0.0):
        """``rollout`` with every seat on the search agent (``crl_ttt_rollout_mcts``): self-play of the search in one launch,
        with the same statistics tensors, ``results()`` rows and step counter."""
        S, R, cexp = self._search_args(simulations, playouts, exploration)
        noise = _unit("noise", noise)
        self._call("crl_ttt_rollout_mcts", _seed(seed), self.first_env_id, int(steps), S, R, cexp, noise, _ptr(self.occ),
                   _ptr(self.winner), _ptr(self.to_move), self._stats())

    # -- the search valued by the caller's network (PUCT); the contract is with crl_ttt_puct_begin in include/colosseum_hip.h
    PUCT_MAX_CAPACITY = 4095

    def _puct_open(self):
        if getattr(self, "_puct_cap", None) is None:
            raise ValueError("no search is open: call puct_begin(capacity) first")
        return self._puct_tree, self._puct_cap

    def _puct_select_spec(self):
        return dict(self._obs_spec(), mover=(torch.int8, (self.B,)), pending=(torch.uint8, (self.B,)),
                    leaf_occ=(torch.int32, (self.P, self.B)))

    def _puct_root_spec(self):
        i32, Bc = torch.int32, (self.B, self.n_cells)
        return {"visits": (i32, Bc), "value": (i32, Bc), "prior": (i32, Bc), "nodes": (i32, (self.B,)), "sims": (i32, (self.B,)),
                "best": (i32, (self.B,))}

    def puct_begin(self, capacity: int):
        """Opens a search of at most ``capacity`` (1 .. 4095) simulations from every game's position (``crl_ttt_puct_begin``):
        the trees live in a device tensor of this stepper, allocated here or reused when the capacity is the last one's, and
        hold their own copy of the position -- the batch may be stepped while the search is open.  Finished positions make
        skipped trees.  One launch, no host synchronisation."""
        cap = _int_in("capacity", capacity, 1, self.PUCT_MAX_CAPACITY)
        if getattr(self, "_puct_cap", None) != cap:
            nbytes = self._lib.crl_ttt_puct_tree_bytes(self._ctx.handle, cap)
            if nbytes < 0:
                check(int(nbytes), "crl_ttt_puct_tree_bytes")
            with torch.cuda.device(self.device):
                self._puct_tree = torch.empty((self.B, int(nbytes) // 16, 2), dtype=torch.int64, device=self.device)   # (16-byte units)
            self._puct_cap = cap
        self._call("crl_ttt_puct_begin", _ptr(self.occ), _ptr(self.winner), _ptr(self.to_move), cap, _ptr(self._puct_tree))

    def puct_select(self, exploration: float = 1.25, fpu: float = 0.5, rel_mod: Optional[int] = None, out: Optional[dict] = None):
        """One descent of every open tree (``crl_ttt_puct_select``): ``exploration`` is c of the PUCT score (0 .. 65535 / 256),
        ``fpu`` the value in [0, 1] of a child without a visit.  Returns the leaves that wait for the caller's network:
        {'board' int8 [B, cells] relative to the leaf's mover, 'valid' int32 [B] empties mask, 'mover' int8 [B], 'pending'
        uint8 [B], 'leaf_occ' int32 [P, B] the leaf position in the state layout}; rows whose tree has no pending leaf (skipped,
        a terminal leaf, at capacity) are zeros with mover -1.  ``out`` reuses such a dict.  One launch, no host synchronisation."""
        tree, cap = self._puct_open()
        cpuct = _exploration("exploration", exploration)
        fpu16 = int(round(65536.0 * _unit("fpu", fpu)))
        rel = self.P if rel_mod is None else _int_in("rel_mod", rel_mod, 1, 127)
        out = _out_dict(out, self._puct_select_spec(), self.device)
        self._call("crl_ttt_puct_select", _ptr(tree), cap, cpuct, fpu16, rel, _ptr(out["board"]), _ptr(out["valid"]),
                   _ptr(out["mover"]), _ptr(out["pending"]), _ptr(out["leaf_occ"]), 0)
        return out

    def puct_backup(self, prior: torch.Tensor, value: torch.Tensor):
        """Expands the pending leaves with ``prior`` (uint16 [B, cells], or int16 of the same bits: any weights, normalised
        over the leaf's empty cells) and backs ``value`` up (int32 [B, P]: the value on 0 .. 65536 of the leaf's mover, then of
        the players after it in turn order); terminal leaves back their outcome up (``crl_ttt_puct_backup``).  One launch."""
        tree, cap = self._puct_open()
        if not isinstance(prior, torch.Tensor) or prior.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
            raise ValueError("prior must be a uint16 (or int16) tensor of shape (%d, %d)" % (self.B, self.n_cells))
        _want(prior, prior.dtype, (self.B, self.n_cells), self.device, "prior")
        if not isinstance(value, torch.Tensor):
            raise ValueError("value must be an int32 tensor of shape (%d, %d)" % (self.B, self.P))
        _want(value, torch.int32, (self.B, self.P), self.device, "value")
        self._call("crl_ttt_puct_backup", _ptr(tree), cap, _ptr(prior), _ptr(value), 0)

    def puct_root(self, out: Optional[dict] = None):
        """The root of every open tree (``crl_ttt_puct_root``): {'visits', 'value', 'prior' int32 [B, cells]: simulations through
        the root's child at each cell, its summed value for the root's mover (65536 per won simulation) and the root's stored
        priors, 'nodes', 'sims', 'best' int32 [B]: the most visited cell (ties: the larger value, then the lowest cell; -1
        without a visited child)}.  The visit counts are the policy target of an AlphaZero-style trainer.  One launch."""
        tree, cap = self._puct_open()
        out = _out_dict(out, self._puct_root_spec(), self.device)
        self._call("crl_ttt_puct_root", _ptr(tree), cap, _ptr(out["visits"]), _ptr(out["value"]), _ptr(out["prior"]),
                   _ptr(out["nodes"]), _ptr(out["sims"]), _ptr(out["best"]))
        return out

    @staticmethod
    def puct_quantize(policy: torch.Tensor, value: torch.Tensor):
        """(float policy [B, cells]: any non-negative weights, float value [B, P] in [0, 1]) -> (int16 prior holding the
        contract's uint16 bits, int32 value on 0 .. 65536) for ``puct_backup``.  Each row's weights are scaled so that its
        greatest is 65535 (the backup normalises over the empty cells anyway); NaN counts as 0.  Torch operations only."""
        pol = torch.nan_to_num(policy.to(torch.float32), nan=0.0, posinf=0.0).clamp_min(0.0)
        top = pol.amax(dim=1, keepdim=True).clamp_min(1e-30)
        q = torch.round(pol * (65535.0 / top)).to(torch.int32).clamp(0, 65535)
        prior = torch.where(q >= 32768, q - 65536, q).to(torch.int16)
        val = torch.round(torch.nan_to_num(value.to(torch.float32), nan=0.5).clamp(0.0, 1.0) * 65536.0).to(torch.int32)
        return prior.contiguous(), val.contiguous()

    def puct(self, evaluate, simulations: int, exploration: float = 1.25, fpu: float = 0.5, out: Optional[dict] = None):
        """A whole search: ``puct_begin(simulations)``, then ``simulations`` times ``puct_select`` -> ``evaluate(leaves)`` ->
        ``puct_backup``, then ``puct_root``.  ``evaluate`` takes the select dict and returns (prior, value), either the integer
        tensors of ``puct_backup`` or float tensors (then ``puct_quantize`` turns them).  Two launches per simulation beside the
        caller's network; no host synchronisation.  Returns the root dict (``out`` reuses one)."""
        if not callable(evaluate):
            raise ValueError("evaluate must be callable: the select dict -> (prior, value)")
        S = _int_in("simulations", simulations, 1, self.PUCT_MAX_CAPACITY)
        _exploration("exploration", exploration), _unit("fpu", fpu)
        self.puct_begin(S)
        leaves = None
        for _ in range(S):
            leaves = self.puct_select(exploration, fpu, out=leaves)
            prior, value = evaluate(leaves)
            if prior.is_floating_point() or value.is_floating_point():
                prior, value = self.puct_quantize(prior, value)
            self.puct_backup(prior, value)
        return self.puct_root(out)

    def puct_action(self, evaluate, simulations: int, exploration: float = 1.25, fpu: float = 0.5,
                    out: Optional[dict] = None) -> torch.Tensor:
        """``puct``'s most visited cell as an int64 [B] action for ``step_single`` (-1 where the game is over)."""
        return self.puct(evaluate, simulations, exploration, fpu, out)["best"].to(torch.int64)

    def rollout(self, steps: int, seed: int = 0):
        self._rollout_plan(steps, seed)

    def results(self, copy: bool = True):
        """int32 [B, 3+P] = n_episodes, len_sum, draw_count, win_count[P]; written by the rollout kernel at the end of
        every launch.  A snapshot by default; ``copy=False`` hands out the live buffer the next rollout rewrites."""
        return self._results.clone() if copy else self._results

    def results_from_columns(self):
        cols = [self.n_episodes, self.len_sum, self.draw_count] + [self.win_count[p] for p in range(self.P)]
        return torch.stack(cols, dim=1).contiguous()


class TTTBoards(_Stepper):
    """B TicTacToe games held in the REFERENCE's layout (``board int8 [B, cells]`` with -1 = empty, ``winner``,
    ``to_move``) and stepped there by ``crl_ttt_step_board`` / ``crl_ttt_observe_board`` -- what the single-state
    drop-in classes run at B = 1; `TTTBatch` (bit masks) is the layout for throughput."""

    def __init__(self, dims: Sequence[int] = (3, 3), k: int = 3, num_players: int = 2, batch: int = 1, device="cuda"):
        self.dims = tuple(int(d) for d in dims)
        d3 = (1,) * (3 - len(self.dims)) + self.dims
        self.K, self.P, self.B = int(k), int(num_players), int(batch)
        self.n_cells = d3[0] * d3[1] * d3[2]
        self._open(device, 0, "crl_ttt_create", d3[0], d3[1], d3[2], self.K, self.P)
        dev, B = self.device, self.B
        self.board = torch.full((B, self.n_cells), -1, dtype=torch.int8, device=dev)
        self.winner = torch.full((B,), -1, dtype=torch.int8, device=dev)
        self.to_move = torch.zeros((B,), dtype=torch.int8, device=dev)
        self.reward = torch.zeros((B,), dtype=torch.int8, device=dev)
        self.terminal = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.winners = torch.zeros((B,), dtype=torch.int8, device=dev)
        self.valid = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.obs = torch.zeros((B, self.n_cells), dtype=torch.int8, device=dev)

    def step(self, action: torch.Tensor, auto_reset: bool = False, rel_mod: Optional[int] = None):
        _want(action, torch.int8, (self.B,), self.device, "action")
        self._call("crl_ttt_step_board", _ptr(self.board), _ptr(self.winner), _ptr(self.to_move), _ptr(action), _ptr(self.reward),
                   _ptr(self.terminal), _ptr(self.winners), _ptr(self.valid), _ptr(self.obs),
                   int(rel_mod if rel_mod else self.P), CRL_STEP_AUTO_RESET if auto_reset else 0)
        return self.reward, self.terminal, self.winners

    def observe(self, player: Optional[torch.Tensor] = None, rel_mod: Optional[int] = None):
        """(obs int8 [B, cells] relative to player[b] -- absolute when player is None --, empties mask int32 [B])"""
        if player is not None:
            _want(player, torch.int8, (self.B,), self.device, "player")
        obs = torch.empty_like(self.board)
        valid = torch.empty_like(self.valid)
        self._call("crl_ttt_observe_board", _ptr(self.board), _ptr(player), int(rel_mod if rel_mod else self.P), _ptr(obs),
                   _ptr(valid))
        return obs, valid


class BlokusBatch(_RolloutStepper):
    """B games of 4-player 20x20 Blokus (reference: envs/blokus/*).

    State tensors (device): occ int32 [B, 4, 20] row bitboards per colour; inv int32 [B, 4] piece masks;
    score int32 [B, 4]; round int32 [B]; to_move int32 [B].  Actions are dense ids
    ``((piece*400 + y*20 + x)*8 + orientation)*5 + shift`` (-1 = pass), see ``envs.blokus.actions``.
    """
    MASK_WORDS = 10500
    STATS_STRUCT = _native.BlokusStats
    PLAN_BIND = "crl_blokus_rollout_bind"
    STATS = {"tcount": (torch.int32, _per_game), "tstep": (torch.int32, _per_game), "n_episodes": (torch.int32, _per_game),
             "win_count": (torch.int32, _per_player), "len_sum": (torch.int32, _per_game), "score_sum": (torch.int32, _per_player),
             "results": (torch.int32, lambda B, P: (B, 10))}

    def __init__(self, batch: int = 1, device="cuda", first_env_id: int = 0):
        self.B = int(batch)
        self.P = 4
        self._open(device, first_env_id, "crl_blokus_create")
        dev, B = self.device, self.B
        with torch.cuda.device(dev):
            self.occ = torch.zeros((B, 4, 20), dtype=torch.int32, device=dev)
            self.inv = torch.zeros((B, 4), dtype=torch.int32, device=dev)
            self.score = torch.zeros((B, 4), dtype=torch.int32, device=dev)
            self.round = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.to_move = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.reward = torch.zeros((B,), dtype=torch.int8, device=dev)
            self.terminal = torch.zeros((B,), dtype=torch.uint8, device=dev)
            self.winners = torch.zeros((B,), dtype=torch.uint8, device=dev)
            self.__dict__.update(_alloc(self._stat_spec(B, 4), dev, torch.zeros))
        self.reset()
        self._open_wait()

    def _state(self):
        return (_ptr(self.occ), _ptr(self.inv), _ptr(self.score), _ptr(self.round), _ptr(self.to_move))

    def reset(self, mask: Optional[torch.Tensor] = None):
        if mask is not None:
            _want(mask, torch.uint8, (self.B,), self.device, "mask")
        self._call("crl_blokus_reset", _ptr(mask), *self._state())

    def step(self, action: torch.Tensor, auto_reset: bool = False):
        _want(action, torch.int32, (self.B,), self.device, "action")
        self._call("crl_blokus_step", *self._state(), _ptr(action), _ptr(self.reward), _ptr(self.terminal), _ptr(self.winners),
                   CRL_STEP_AUTO_RESET if auto_reset else 0)
        return self.reward, self.terminal, self.winners

    def valid(self, player: Optional[torch.Tensor] = None, want_mask: bool = False):
        """Legal-action count int32 [B] of `player` (default: the player to move) and, on request, the dense
        id bitmap int32 [B, 10500] (bit id set = legal; ascending ids = the reference's valid_actions order)."""
        if player is not None:
            _want(player, torch.int8, (self.B,), self.device, "player")
        count = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        mask = torch.empty((self.B, self.MASK_WORDS), dtype=torch.int32, device=self.device) if want_mask else None
        self._call("crl_blokus_valid", *self._state(), _ptr(player), _ptr(count), _ptr(mask))
        return (count, mask) if want_mask else count

    def valid_list(self, cap: int = 2048, player: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        """The ordered legal-action LIST of `player` (default: the player to move), compacted: (count int32 [B],
        ids int32 [B, cap]) with ``ids[b, :min(count[b], cap)]`` = the dense ids in ascending order = the reference's
        ``valid_actions`` order (BlokusEnvironment.py:453-500); entries beyond are -1 (or whatever `out` held)."""
        if player is not None:
            _want(player, torch.int8, (self.B,), self.device, "player")
        count = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        ids = out if out is not None else torch.full((self.B, int(cap)), -1, dtype=torch.int32, device=self.device)
        _want(ids, torch.int32, (self.B, int(cap)), self.device, "out")
        self._call("crl_blokus_valid_list", *self._state(), _ptr(player), _ptr(ids), _ptr(count), int(cap))
        return count, ids

    def select(self, rank: torch.Tensor, player: Optional[torch.Tensor] = None):
        """Dense id of the rank[b]-th legal action (reference order) of `player` (default: the player to move) without
        materialising the list; -1 where rank is outside [0, count).  -> (action int32 [B], count int32 [B])."""
        _want(rank, torch.int32, (self.B,), self.device, "rank")
        if player is not None:
            _want(player, torch.int8, (self.B,), self.device, "player")
        act = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        count = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        self._call("crl_blokus_select", *self._state(), _ptr(player), _ptr(rank), _ptr(act), _ptr(count))
        return act, count

    def is_valid(self, action: torch.Tensor, player: Optional[torch.Tensor] = None):
        """``is_valid_action`` for all games: uint8 [B], 1 iff the dense id action[b] is a legal action of `player`."""
        _want(action, torch.int32, (self.B,), self.device, "action")
        if player is not None:
            _want(player, torch.int8, (self.B,), self.device, "player")
        ok = torch.empty((self.B,), dtype=torch.uint8, device=self.device)
        self._call("crl_blokus_is_valid", *self._state(), _ptr(player), _ptr(action), _ptr(ok))
        return ok

    def fits(self, action: torch.Tensor, player: torch.Tensor):
        """uint8 [B]: 1 iff every cell of the placement action[b] lies on the board, is empty and has no orthogonal neighbour
        of player[b]'s colour -- ``is_valid`` without the anchor and inventory conditions (one shift of the reference's
        ``Board.check_orientation_shifts``)."""
        _want(action, torch.int32, (self.B,), self.device, "action")
        _want(player, torch.int8, (self.B,), self.device, "player")
        ok = torch.empty((self.B,), dtype=torch.uint8, device=self.device)
        self._call("crl_blokus_fits", _ptr(self.occ), _ptr(player), _ptr(action), _ptr(ok))
        return ok

    def set_board(self, board: torch.Tensor):
        """Loads ``Board.board_contents`` (int8 [B, 20, 20], 0 empty else colour) into the row bitboards."""
        _want(board, torch.int8, (self.B, 20, 20), self.device, "board")
        self._call("crl_blokus_pack", _ptr(board), _ptr(self.occ))

    def sample(self, seed: int = 0, advance: bool = True):
        """The rollout's random agent for one step: int32 [B] dense action id of a uniformly drawn legal action of the
        player to move (-1 = pass); ``step(sample(seed), auto_reset=True)`` T times == ``rollout(T, seed)``."""
        act = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        self._call("crl_blokus_sample", _seed(seed), self.first_env_id, *self._state(), _ptr(self.tcount), int(advance), _ptr(act))
        return act

    def observe(self, player: torch.Tensor):
        """state_to_observation for all games; player int8 [B] is the observer of each game."""
        _want(player, torch.int8, (self.B,), self.device, "player")
        ob = torch.empty((self.B, 20, 20), dtype=torch.int8, device=self.device)
        op = torch.empty((self.B, 4, 21), dtype=torch.uint8, device=self.device)
        osc = torch.empty((self.B, 4), dtype=torch.int32, device=self.device)
        self._call("crl_blokus_observe", _ptr(self.occ), _ptr(self.inv), _ptr(self.score), _ptr(player), _ptr(ob), _ptr(op),
                   _ptr(osc))
        return {"board": ob, "pieces": op, "score": osc, "player": player.view(self.B, 1)}

    def _obs_spec(self):
        """the buffers `step_observe` and `step_single` fill for the next mover / the learner"""
        return {"board": (torch.int8, (self.B, 20, 20)), "pieces": (torch.uint8, (self.B, 4, 21)),
                "score": (torch.int32, (self.B, 4)), "n_valid": (torch.int32, (self.B,))}

    def step_observe(self, action: Optional[torch.Tensor] = None, seed: int = 0, auto_reset: bool = True,
                     out: Optional[dict] = None, list_cap: int = 0):
        """One ply of every game in ONE launch: plays `action` (int32 [B] dense ids; None = the rollout's random agent
        at each game's step counter, which then advances) and returns what the next mover needs:
        {'board' int8 [B, 20, 20], 'pieces' uint8 [B, 4, 21], 'score' int32 [B, 4], 'player' int8 [B, 1] (its observation),
        'n_valid' int32 [B] (its number of legal actions), 'reward', 'terminal', 'winners'}.
        Equals ``step(...); valid(); observe(to_move)``.
        ``list_cap`` > 0 queues ``valid_list(list_cap)`` for the next mover right behind it (same stream, no synchronise in
        between) and adds 'ids' int32 [B, list_cap]: the ordered legal ids a policy picks from (-1 beyond 'n_valid')."""
        if action is not None:
            _want(action, torch.int32, (self.B,), self.device, "action")
        out = out or _alloc(dict(self._obs_spec(), player=(torch.int8, (self.B, 1))), self.device)
        self._call("crl_blokus_step_observe", _seed(seed), self.first_env_id, *self._state(), _ptr(action), _ptr(self.tcount),
                   _ptr(self.reward), _ptr(self.terminal), _ptr(self.winners), _ptr(out["n_valid"]), _ptr(out["board"]),
                   _ptr(out["pieces"]), _ptr(out["score"]), _ptr(out["player"]), CRL_STEP_AUTO_RESET if auto_reset else 0)
        out["reward"], out["terminal"], out["winners"] = self.reward, self.terminal, self.winners
        if list_cap > 0:
            ids = out.get("ids")
            if ids is None or tuple(ids.shape) != (self.B, int(list_cap)):
                ids = torch.empty((self.B, int(list_cap)), dtype=torch.int32, device=self.device)
            ids.fill_(-1)
            out["ids"] = self.valid_list(int(list_cap), out=ids)[1]
        return out

    OPPONENTS = ("random", "mcts")          # who `step_single` seats

    def step_single(self, seat: torch.Tensor, learner_action: Optional[torch.Tensor] = None, seed: int = 0,
                    rank: bool = False, out: Optional[dict] = None, opponent: str = "random", noise: float = 0.0,
                    simulations: int = 64, playouts: int = 1, width: int = 8, exploration: float = 1.0):
        """One step of "learner at seat[b] against the random agent" in every game, ONE launch (``crl_blokus_step_single``):
        the learner plays ``learner_action`` (int64 [B]: a dense or extended id, < 0 = pass; with ``rank=True`` the index
        into its ordered legal list, outside [0, count) = pass) when it is its turn, the random agent plays the other
        seats until it is the learner's turn again, finished games restart on the way.  ``learner_action=None`` only
        advances to the learner's turn.  seat int8 [B].  Returns {'board', 'pieces', 'score' (the learner's observation),
        'n_valid' int32 [B] (its number of legal actions), 'reward' int8 [B] (its final rank when a game ended, else 0, or
        a ``CRL_BLOKUS_*_ERROR`` code for an action the reference's next_state raises on -- that game then stays as it
        was), 'done' uint8 [B], 'winners' uint8 [B]}; every ply, the learner's included, advances ``tcount``.
        ``opponent="mcts"``: every other seat plays the search agent (``crl_blokus_step_single_mcts``; ``sample_mcts``'s moves)
        with ``simulations``, ``playouts``, ``width``, ``exploration`` and ``noise``; still one launch.  The keywords are
        checked for either opponent and used only with that one."""
        _want(seat, torch.int8, (self.B,), self.device, "seat")
        if learner_action is not None:
            _want(learner_action, torch.int64, (self.B,), self.device, "learner_action")
        opponent = _one_of("opponent", opponent, self.OPPONENTS)
        search = self._agent_args(simulations, playouts, width, exploration, noise)
        name, tail = ("crl_blokus_step_single_mcts", search) if opponent == "mcts" else ("crl_blokus_step_single", ())
        out = out or _alloc(dict(self._obs_spec(), done=(torch.uint8, (self.B,))), self.device)
        self._call(name, _seed(seed), self.first_env_id, *self._state(), _ptr(seat), _ptr(learner_action),
                   _ptr(self.tcount), _ptr(self.reward), _ptr(out["done"]), _ptr(self.winners), _ptr(out["n_valid"]),
                   _ptr(out["board"]), _ptr(out["pieces"]), _ptr(out["score"]), *tail, CRL_STEP_RANK_ACTION if rank else 0)
        out["reward"], out["winners"] = self.reward, self.winners
        return out

    def playout(self, playouts: int, candidates: Optional[torch.Tensor] = None, seed: int = 0, out: Optional[dict] = None):
        """Random playouts from every game's position, ONE launch (``crl_blokus_playout``): row (b, a) plays the dense id
        ``candidates[b, a]`` (int32 [B, A]; anything that is not a legal action of the player to move skips the row) and
        then ``playouts`` random games to their end, on private copies; ``candidates=None`` evaluates the position as it
        stands (A = 1).  The draws are keyed by ``seed``, the game ids and ``tcount`` as the counter base (which the call
        neither advances nor writes; the state is only read).  Returns {'wins' int32 [B, A, 4] (a shared best score
        counts for every tied player), 'draws' (played - sum of wins, negative when ties count twice), 'played',
        'len_sum' int32 [B, A], 'score_sum' int32 [B, A, 4]} (skipped rows are zeros); ``out`` reuses such a dict.  No
        host synchronisation; capturable into a graph."""
        R = _int_in("playouts", playouts, 1, 65535)
        A = _candidates(candidates, self.B, self.device, 65535)
        i32, BA = torch.int32, (self.B, A)
        out = _out_dict(out, {"wins": (i32, BA + (4,)), "draws": (i32, BA), "played": (i32, BA), "len_sum": (i32, BA),
                              "score_sum": (i32, BA + (4,))}, self.device)
        self._call("crl_blokus_playout", _seed(seed), self.first_env_id, *self._state(), _ptr(self.tcount), _ptr(candidates), A, R,
                   _ptr(out["wins"]), _ptr(out["played"]), _ptr(out["len_sum"]), _ptr(out["score_sum"]), 0)
        torch.sub(out["played"], out["wins"].sum(dim=2, dtype=torch.int32), out=out["draws"])
        return out

    def flat_mc_action(self, candidates: torch.Tensor, playouts: int, seed: int = 0, out: Optional[dict] = None) -> torch.Tensor:
        """Flat Monte Carlo over the dense-id ``candidates`` (int32 [B, A]) of the player to move: ``playout`` on each,
        value = the mover's wins, the best candidate (ties: the lower index) as an int64 [B] action for ``step_single``;
        -1 where no candidate was played.  ``out``: the playout dict to reuse.  No host synchronisation; capturable."""
        _int_in("playouts", playouts, 1, 65535)
        A = _candidates(candidates, self.B, self.device, 65535)
        o = self.playout(playouts, candidates, seed, out)
        mover = (self.to_move.to(torch.int64) & 3).view(-1, 1, 1).expand(self.B, A, 1)
        return _flat_mc_pick(torch.gather(o["wins"], 2, mover).squeeze(2), o["played"], candidates)

    # -- tree search with progressive widening; the contract is with crl_blokus_mcts in include/colosseum_hip.h
    @functools.cached_property
    def mcts_max_simulations(self) -> int:
        """the most simulations ``mcts`` takes (``crl_blokus_mcts_max_simulations``: the tree stays in LDS)"""
        rc = self._lib.crl_blokus_mcts_max_simulations(self._ctx.handle)
        if rc < 0:
            check(rc, "crl_blokus_mcts_max_simulations")
        return int(rc)

    def mcts(self, simulations: int, playouts: int = 1, candidates: Optional[torch.Tensor] = None, width: int = 8, seed: int = 0,
             exploration: float = 1.0, out: Optional[dict] = None):
        """A tree search for the player to move in every game, ONE launch (``crl_blokus_mcts``): each game builds a tree of
        its own by ``simulations`` descents (at most ``mcts_max_simulations``), each new leaf valued by ``playouts`` (1 ..
        1024) random games to their end.  A node is widened progressively: it gets its k-th child, a uniformly drawn legal
        action, once it has about k^2 visits, up to ``width`` (1 .. 64) children.  With ``candidates`` (int32 [B, A], A <= 64
        dense ids) the root's children are the legal, distinct candidates instead, slot = column; the nodes below widen.
        ``exploration`` (0 .. 65535 / 256; 0 = pure exploitation) multiplies sqrt(log2 n_parent / n_child) on a value scale
        of 0 .. 1.  The draws are keyed by ``seed``, the game ids and ``tcount`` as the counter base (the call reads the state
        and writes none of it).  Returns {'ids' int32 [B, K]: the dense id of the root's child in each slot (-1 the pass, -2
        an empty slot; K = A with candidates, else ``width``), 'visits', 'value' int32 [B, K]: simulations through that child
        and the playouts the mover won behind it, 'nodes' int32 [B], 'best' int32 [B]: the id of the most visited child
        (ties: the larger value, then the lowest slot; -2 where no candidate was playable)}; ``out`` reuses such a dict.  No
        host synchronisation; capturable into a graph."""
        S = _int_in("simulations", simulations, 1, self.mcts_max_simulations)
        R = _int_in("playouts", playouts, 1, 1024)
        A = _candidates(candidates, self.B, self.device, 64)
        W = _int_in("width", width, 1, 64)
        cexp = _exploration("exploration", exploration)
        i32, BK = torch.int32, (self.B, A if candidates is not None else W)
        out = _out_dict(out, {"ids": (i32, BK), "visits": (i32, BK), "value": (i32, BK), "nodes": (i32, (self.B,)),
                              "best": (i32, (self.B,))}, self.device)
        self._call("crl_blokus_mcts", _seed(seed), self.first_env_id, *self._state(), _ptr(self.tcount), _ptr(candidates), A, W, S, R,
                   cexp, _ptr(out["ids"]), _ptr(out["visits"]), _ptr(out["value"]), _ptr(out["nodes"]), _ptr(out["best"]), 0)
        return out

    def mcts_action(self, simulations: int, playouts: int = 1, candidates: Optional[torch.Tensor] = None, width: int = 8,
                    seed: int = 0, exploration: float = 1.0, out: Optional[dict] = None) -> torch.Tensor:
        """``mcts``'s most visited child as an int64 [B] action for ``step_single`` (-1 = pass, also where no candidate was
        playable).  No host synchronisation; capturable."""
        return self.mcts(simulations, playouts, candidates, width, seed, exploration, out)["best"].to(torch.int64).clamp_(min=-1)

    # -- the search as a seated agent; the contract is with crl_blokus_sample_mcts in include/colosseum_hip.h
    def _agent_args(self, simulations, playouts, width, exploration, noise):
        """(W, S, R, cexp, noise) of the search agent as the C entries take them, checked"""
        S = _int_in("simulations", simulations, 1, self.mcts_max_simulations)
        R = _int_in("playouts", playouts, 1, 1024)
        W = _int_in("width", width, 1, 64)
        return (W, S, R, _exploration("exploration", exploration), _unit("noise", noise))

    def sample_mcts(self, simulations: int, playouts: int = 1, width: int = 8, seed: int = 0, exploration: float = 1.0,
                    noise: float = 0.0, advance: bool = True):
        """The search agent for one step (``crl_blokus_sample_mcts``): int32 [B] dense id at each game's step counter -- -1
        (pass) for a mover without actions, with probability ``noise`` the random agent's action (``sample``'s draw: at
        ``noise=1`` the same move), else ``best`` of ``mcts(simulations, playouts, None, width, seed, exploration)`` on the
        position with the counter as its base.  ``step(sample_mcts(...), auto_reset=True)`` T times == ``rollout_mcts(T,
        ...)``.  One launch; no host synchronisation, capturable into a graph."""
        search = self._agent_args(simulations, playouts, width, exploration, noise)
        act = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        self._call("crl_blokus_sample_mcts", _seed(seed), self.first_env_id, *self._state(), _ptr(self.tcount), int(advance),
                   *search, _ptr(act))
        return act

    def rollout_mcts(self, steps: int, simulations: int, playouts: int = 1, width: int = 8, seed: int = 0,
                     exploration: float = 1.0, noise: float = 0.0):
        """``rollout`` with every seat on the search agent (``crl_blokus_rollout_mcts``): self-play of the search in one
        launch, with the same statistics tensors, ``results()`` rows and step counter."""
        search = self._agent_args(simulations, playouts, width, exploration, noise)
        self._call("crl_blokus_rollout_mcts", _seed(seed), self.first_env_id, int(steps), *search, *self._state(), self._stats())

    def board(self):
        out = torch.empty((self.B, 20, 20), dtype=torch.int8, device=self.device)
        self._call("crl_blokus_board", _ptr(self.occ), _ptr(out))
        return out

    def rollout(self, steps: int, seed: int = 0):
        self._rollout_plan(steps, seed)

    def results(self, copy: bool = True):
        """int32 [B, 10] = n_episodes, len_sum, win_count[4], score_sum[4]; written by the rollout kernel at the end of
        every launch.  A snapshot by default; ``copy=False`` hands out the live buffer the next rollout rewrites."""
        return self._results.clone() if copy else self._results

    def results_from_columns(self):
        cols = [self.n_episodes, self.len_sum] + [self.win_count[p] for p in range(4)] + [self.score_sum[p] for p in range(4)]
        return torch.stack(cols, dim=1).contiguous()
