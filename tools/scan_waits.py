#!/usr/bin/env python3
"""Scan the device assembly of the library for loads that wait alone.

For every kernel, count the global/buffer loads followed directly (before any
other load) by an `s_waitcnt vmcnt(0)`, and the flat / scratch memory
instructions.  A gather whose loads each wait alone, or that goes through
flat loads (they count against lgkmcnt too, so every LDS wait drains them),
shows up here.

    python tools/scan_waits.py [--min 6]

--store-waits lists another pattern instead: a prefetch that is drained in
front of stores.  Per kernel, every `s_waitcnt vmcnt(N)` that follows a run of
k >= 4 consecutive global loads with N < k, and is itself followed by a global
store with no other global load between (k_scatter_res, DESIGN.md §4: the
loads of the next tile were waited for before the segment stores of this one).

    python tools/scan_waits.py --store-waits [--files partition.hip bucketsort.hip]
    python tools/scan_waits.py --store-waits --asm some.s other.s

Compiles csrc/*.hip for gfx950 with --cuda-device-only -S into /tmp, or reads
the assembly files given with --asm.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avx-sort-merge-joins_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
MIN_RUN = 4  # --store-waits: the shortest run of loads that counts as a prefetch

_KERNEL = re.compile(r"^(_Z\S+):\s*;\s*@")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def scan(path):
    fn, prev = None, None
    waits, flat = {}, {}
    for line in open(path):
        m = _KERNEL.match(line)
        if m:
            fn, prev = m.group(1), None
            continue
        if fn is None:
            continue
        t = line.strip()
        if t.startswith(("flat_", "scratch_")):
            flat[fn] = flat.get(fn, 0) + 1
        if t.startswith(("global_load", "buffer_load")):
            prev = "L"
        elif t.startswith("s_waitcnt") and "vmcnt(0)" in t:
            if prev == "L":
                waits[fn] = waits.get(fn, 0) + 1
            prev = "W"
    return waits, flat


def scan_store_waits(lines):
    """[(kernel, line number, k, N, the store)] of the assembly text `lines`:
    every `s_waitcnt vmcnt(N)` behind a run of k >= MIN_RUN global loads with
    N < k whose next global memory instruction is a store.

    A run is a sequence of global_load instructions with nothing between them
    but scalar, vector-ALU and LDS instructions: a store, an atomic, a wait on
    vmcnt, a barrier, a branch or a label ends it.  A wait leaves min(k, N)
    loads of the run pending, so a later wait is judged against what is still
    in flight.  Text order stands for program order: the scan does not follow
    branches (the store may sit in a loop behind the wait's block)."""
    found = []
    fn = None
    k = 0           # loads of the latest run still pending
    open_run = False
    cand = []       # waits seen since the run, not yet followed by a load or store
    for no, line in enumerate(lines, 1):
        m = _KERNEL.match(line)
        if m:
            fn, k, open_run, cand = m.group(1), 0, False, []
            continue
        if fn is None:
            continue
        t = line.split(";")[0].strip()
        if not t:
            continue
        if t.startswith("global_load"):
            k = k + 1 if open_run else 1
            open_run = True
            cand = []
        elif t.startswith("global_store"):
            found += [(fn, wno, wk, wn, t.split()[0]) for wno, wk, wn in cand]
            cand, k, open_run = [], 0, False
        elif t.startswith(("global_atomic", "buffer_", "flat_", "scratch_")):
            open_run = False
        elif t.startswith("s_waitcnt"):
            m = _VMCNT.search(t)
            if m:
                n = int(m.group(1))
                if k >= MIN_RUN and n < k:
                    cand.append((no, k, n))
                k = min(k, n)
                open_run = False
        elif t.startswith(("s_barrier", "s_cbranch", "s_branch", "s_endpgm")) or t.endswith(":"):
            open_run = False
    return found


def _compile(f, d):
    out = f"/tmp/scan_{f}{d}.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950",
                    "--cuda-device-only", "-S", *([d] if d else []),
                    os.path.join(CSRC, f), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    return out


def _demangled(names):
    """{mangled: demangled} through c++filt where it exists."""
    names = sorted(set(names))
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                             text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def report_store_waits(tag, path):
    with open(path) as f:
        found = scan_store_waits(f)
    names = _demangled(x[0] for x in found)
    for fn, no, k, n, store in found:
        print(f"{tag:28s} line {no:7d}  {k:2d} loads, vmcnt({n}) before {store}  "
              f"{names[fn][:140]}")
    print(f"{tag:28s} {len(found)} wait(s) in {len(set(x[0] for x in found))} kernel(s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min", type=int, default=6, help="report kernels with at least this many")
    ap.add_argument("--store-waits", action="store_true",
                    help="list waits that drain a run of loads in front of a store")
    ap.add_argument("--files", nargs="+", default=None, help="sources of csrc/ (default: all)")
    ap.add_argument("--asm", nargs="+", default=None, help="scan these assembly files instead")
    a = ap.parse_args()
    if a.asm:
        todo = [(os.path.basename(p), p) for p in a.asm]
    else:
        todo = []
        for f in a.files or sorted(os.listdir(CSRC)):
            if not f.endswith(".hip"):
                continue
            for d in ("", "-DKEY_8B"):
                todo.append((f + (" (16 B)" if d else " (8 B)"), _compile(f, d)))
    for tag, out in todo:
        if a.store_waits:
            report_store_waits(tag, out)
            continue
        waits, flat = scan(out)
        for k, v in sorted(waits.items(), key=lambda x: -x[1]):
            if v >= a.min:
                print(f"{tag:28s} lone waits {v:4d}  {k[:100]}")
        for k, v in sorted(flat.items(), key=lambda x: -x[1]):
            print(f"{tag:28s} flat/scratch {v:3d}  {k[:100]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
