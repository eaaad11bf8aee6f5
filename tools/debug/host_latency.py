#!/usr/bin/env python3
"""Host-side cost of the pieces of the contract's timed region (one 20-step Tron launch + gather + synchronise), warm:
the raw ctypes call, TronBatch.rollout, ShardedRollout.rollout, the gather without a process group, an idle synchronise,
and the whole region against ctypes call + synchronise alone (what the Python layers above the C ABI add: ~1.3 us).
Then the three forms of the launch itself -- the 12-argument rollout entry through ctypes, a bound plan through ctypes, the
plan through the C-API entry (colosseumrl_amd._crl_fast) -- twice: the host time of the launching call alone (T = 20, the
queue drained outside the clock), and the call overhead with nothing launched (T = 0: marshalling, checks and return; best
of 7 x 20,000 calls).  Writes what it measured to profiles/launch_path.json, key `host_latency` (--out PATH for another place).
    python tools/debug/host_latency.py [--out PATH]"""
import sys
if "-h" in sys.argv[1:] or "--help" in sys.argv[1:]:     # usage without touching the GPU (tests/test_tools_smoke.py)
    print(__doc__)
    sys.exit(0)
import json
import os
import time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv[1:] else os.path.join(ROOT, "profiles", "launch_path.json")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from colosseumrl_amd import _native
from colosseumrl_amd.batched import TronBatch, _stream, _stream_handle, _DevGuard
from colosseumrl_amd.parallel import ShardedRollout
tb = TronBatch(20, 4, 65536)
sr = ShardedRollout(lambda batch, first_env_id: TronBatch(20, 4, batch, first_env_id=first_env_id), 65536)
st = sr.stepper
for _ in range(50):
    st.rollout(20, 0); torch.cuda.synchronize()
def t(fn, n=2000):
    fn()
    t0 = time.perf_counter()
    for _ in range(n): fn()
    return (time.perf_counter() - t0) / n * 1e6
print("perf_counter pair           %.2f us" % t(lambda: time.perf_counter()))
print("_stream()                   %.2f us" % t(_stream))
g = _DevGuard(st.device)
def guard():
    with g: pass
print("_DevGuard enter/exit        %.2f us" % t(guard))
print("torch.cuda.synchronize idle %.2f us" % t(torch.cuda.synchronize))
args = st._rollout_args or st._bind_rollout()
lib = st._lib
s = _stream()
def raw():
    lib.crl_tron_rollout(st._ctx.handle, st.B, 0, st.first_env_id, 20, *args, 0, s)
# launch only (async) then sync outside the timing: measure launch call cost with queue draining every 20
def launch_cost(fn, n=400):
    tot = 0.0
    for i in range(n):
        t0 = time.perf_counter(); fn(); tot += time.perf_counter() - t0
        torch.cuda.synchronize()
    return tot / n * 1e6
print("ctypes crl_tron_rollout     %.2f us" % launch_cost(raw))
print("TronBatch.rollout           %.2f us" % launch_cost(lambda: st.rollout(20, 0)))
print("ShardedRollout.rollout      %.2f us" % launch_cost(lambda: sr.rollout(20, 0, 8192)))
print("sr.gather(copy=False)       %.2f us" % t(lambda: sr.gather(copy=False)))
def region():
    sr.rollout(20, 0, 8192); sr.gather(copy=False); torch.cuda.synchronize()
print("region (rollout+gather+sync) %.2f us" % t(region, 500))
def region_raw():
    raw(); torch.cuda.synchronize()
print("region raw (ctypes+sync)     %.2f us" % t(region_raw, 500))


# ---- the launch itself, three ways
plan = st._plans.get(0) or st._bind_plan(0)
fast = _native.fast()
sh = _stream_handle()
forms = {"ctypes_12_arguments": lambda T: lib.crl_tron_rollout(st._ctx.handle, st.B, 0, st.first_env_id, T, *args, 0, s),
         "ctypes_plan": lambda T: lib.crl_rollout_launch(plan, 0, T, sh)}
if fast is not None:
    forms["fast_plan"] = lambda T: fast.rollout_launch(plan, 0, T, sh)
def best_of(fn, reps=7, n=20000):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(n): fn()
        best = min(best, (time.perf_counter() - t0) / n * 1e6)
    return best
loop_us = best_of(lambda: None)
record = {"what": "host time of one rollout launch call, us; tools/debug/host_latency.py", "device": torch.cuda.get_device_name(0),
          "workload": {"N": 20, "P": 4, "B": st.B, "T": 20}, "empty_lambda_us": round(loop_us, 3), "forms": {}}
for name, fn in forms.items():
    call = best_of(lambda: fn(0)) - loop_us                                  # T = 0: everything but the launch
    launch = launch_cost(lambda: fn(20))
    record["forms"][name] = {"call_overhead_us": round(call, 3), "launch_call_us": round(launch, 3)}
    print("%-22s call overhead (T = 0) %.2f us   launching call (T = 20) %.2f us" % (name, call, launch))
record["stepper_launcher"] = "fast_plan" if st._launch is getattr(fast, "rollout_launch", None) else "ctypes_plan"
record["TronBatch_rollout_us"] = round(launch_cost(lambda: st.rollout(20, 0)), 3)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
try:                                        # the file also keeps the A/B runs of the change (docs/history.md): only this key is rewritten
    with open(OUT) as f:
        doc = json.load(f)
except (OSError, ValueError):
    doc = {}
doc["host_latency"] = record
with open(OUT, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", OUT)
