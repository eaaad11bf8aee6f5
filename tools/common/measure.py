"""What the rate and A/B tools under tools/ share: the two device-event timing forms, the statistics the committed figures
use, the TicTacToe shapes, the JSON-line output, and the runner that gives every library build a child process of its own.

A module, not a script.  Importing it imports no torch and touches no GPU: the functions that time import torch when they
are called, so a tool's --help and the alternating runner's parent process stay off the device.

  isolated(fn, reps, warmup)               one call between two synchronisations (what a caller that waits for every call sees)
  back_to_back(fn, calls, rounds, warmup)  `calls` calls between two events (steady state; launch gaps overlap the kernels)
Both return milliseconds per call, one value per repetition / round; median() and spread() reduce them (the minimum is min()).
"""
import json
import os
import subprocess
import sys

TTT_SHAPES = [((3, 3), 3, 2), ((3, 5), 3, 3), ((3, 3, 3), 3, 4), ((5, 5), 4, 3)]      # (dims, k in a row, players)


def shape_name(dims, k, p):
    return "x".join(map(str, dims)) + "_k%d_p%d" % (k, p)


# ------------------------------------------------------------------ timing (device events, milliseconds per call)
def isolated(fn, reps, warmup=0, wall=False):
    """`warmup` calls, then reps x (synchronise, record, fn(), record, wait for the second event).  wall=True: also the
    host clock from before the first record to after the wait, as a second list"""
    import time
    import torch
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts, walls = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        ts.append(start.elapsed_time(stop))
    return (ts, walls) if wall else ts


def back_to_back(fn, calls, rounds, warmup=0):
    """`warmup` calls and a synchronise, then rounds x (record, calls x fn(), record, synchronise)"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        ts.append(start.elapsed_time(stop) / calls)
    return ts


# ------------------------------------------------------------------ statistics
def median(values):
    """the upper median (of [1, 2, 3, 4]: 3), the one every committed figure uses"""
    return sorted(values)[len(values) // 2]


def spread(values):
    """median, [min, max]"""
    return median(values), [min(values), max(values)]


# ------------------------------------------------------------------ rows and the GPU
def emit(row):
    print(json.dumps(row), flush=True)


def write_rows(path, rows):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


def require_gpu(tool):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("%s needs a GPU" % tool)


# ------------------------------------------------------------------ one child process per library build, builds alternating
class ChildFailed(SystemExit):
    """a child of alternate() gave no result; uncaught, it ends the tool with status 1 and the child's output on stderr"""


def alternate(argv, builds, rounds, timeout, marker, cwd=None):
    """Starts `argv` once per round and build -- tag0, tag1, ..., tag0, tag1, ... over builds = [(tag, library path or None)]
    -- with CRL_LIB_PATH set to the build's library (None: unset, the shipped library), a library being loaded once per
    process.  Yields (tag, result) as each child ends, result being the JSON behind `marker` on the child's last stdout line
    that starts with it.  The first child that exits non-zero, is killed by a signal, outlives `timeout` seconds or prints
    no such line raises ChildFailed with its output, and no further child is started: on a shared card nothing runs after a
    failure.  Refuses to run from a process that holds a GPU context (a fork + exec from one is what the pool forbids)."""
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        raise RuntimeError("alternate(): this process holds a GPU context; start the children from one that does not")
    for _ in range(rounds):
        for tag, lib in builds:
            env = dict(os.environ)
            env.pop("CRL_LIB_PATH", None)
            if lib is not None:
                env["CRL_LIB_PATH"] = os.path.abspath(lib)
            try:
                r = subprocess.run(argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
            except subprocess.TimeoutExpired as e:
                raise ChildFailed("the child of the %s build ran past %g s and was killed:\n%s%s" % (tag, timeout, _text(e.stdout), _text(e.stderr)))
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith(marker)]
            if r.returncode != 0 or not lines:
                raise ChildFailed("the child of the %s build failed (status %d):\n%s%s" % (tag, r.returncode, r.stdout, r.stderr))
            yield tag, json.loads(lines[-1][len(marker):])


def _text(out):
    return out.decode(errors="replace") if isinstance(out, bytes) else out or ""
