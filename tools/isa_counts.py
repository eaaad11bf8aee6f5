#!/usr/bin/env python3
"""Static figures of ONE kernel out of the device assembly hipcc writes:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S colosseumrl_amd/csrc/tron.hip -o tron.s
    python tools/isa_counts.py tron.s tron_rollout_quad_kernel

The kernel is named by a substring of its (mangled) symbol; the first match is taken.  Prints counts only -- code length,
instructions by class (VALU, SALU, LDS, global memory, branches, waits, other), the static index of the first global
load and of the first workgroup barrier, registers, scratch and LDS as the kernel descriptor states them -- as one JSON
line, to be kept next to the profiles (profiles/README.md)."""
import json
import re
import sys


def classify(op):
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_sleep")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    return "other"


def main(argv):
    if len(argv) != 3 or argv[1] in ("-h", "--help"):
        print(__doc__)
        return 0 if len(argv) > 1 and argv[1] in ("-h", "--help") else 2
    lines = open(argv[1]).read().splitlines()
    start = next((i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_][\w$.]*:", l) and argv[2] in l and not l.startswith(".L")), None)
    if start is None:
        print("no kernel matching %r in %s" % (argv[2], argv[1]))
        return 1
    symbol = lines[start].split(":")[0]
    counts = {k: 0 for k in ("valu", "salu", "lds", "global", "branch", "wait", "other")}
    n = 0
    first_load = first_barrier = None
    end = start + 1
    for end in range(start + 1, len(lines)):
        l = lines[end].split(";")[0].strip()
        if l.startswith(".Lfunc_end") or l.startswith(".size"):
            break
        if not l or l.endswith(":") or l.startswith("."):
            continue
        op = l.split()[0]
        counts[classify(op)] += 1
        if first_load is None and op.startswith(("global_load", "flat_load", "buffer_load")):
            first_load = n
        if first_barrier is None and op.startswith("s_barrier"):
            first_barrier = n
        n += 1
    out = {"kernel": symbol, "instructions": n, **counts, "first_global_load": first_load, "first_barrier": first_barrier}
    # the kernel descriptor and the compiler's own summary comments that follow the body
    text = "\n".join(lines[end:end + 400])
    for key, pat in (("code_bytes", r"; codeLenInByte = (\d+)"), ("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"),
                     ("sgprs", r"; NumSgprs: (\d+)"), ("scratch_bytes", r"; ScratchSize: (\d+)"), ("lds_bytes", r"; LDSByteSize: (\d+)"),
                     ("occupancy", r"; Occupancy: (\d+)")):
        m = re.search(pat, text)
        out[key] = int(m.group(1)) if m else None
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
