#!/usr/bin/env python3
"""Time smj_dev_outer_join beside smj_dev_join_pairs and smj_dev_materialize
on the same sorted inputs, in one process (DESIGN.md §7's outer join numbers).

    python tools/time_outer_join.py [--n 134217728] [--widths 16 8] [--reps 11]
                                    [--warmup 3] [--also NAME=DIR ...]
                                    [--out profiles/outer_join_timing.jsonl]

Per tuple width two lines of JSON are printed and appended to --out:

  part "covered"  sorted PK R (keys 1..n) and FK S holding every key once.  No
      tuple lacks a partner, so how="full" writing r_payload, s_payload and
      key gives smj_dev_join_pairs' rows (checked): the ratio of the two is
      the cost of the outer bookkeeping.  Also how="inner", the count-only
      call and smj_dev_outer_join_count.
  part "half"     the same R against n of the keys 1..2n, so about half of
      each side has no partner: how="full" with all five columns, and "left"
      and "right", beside smj_dev_join_pairs of these inputs.

--also NAME=DIR names another build of the libraries (make BUILD=...
LIBOUT=...): its smj_dev_join_pairs and smj_dev_materialize join the
round-robin of part "covered" as join_pairs_NAME / materialize_NAME, so the
parent commit's kernels, or this build loaded a second time, are timed beside
this one's.

The calls run round-robin, each timed with device events (every call but the
count form synchronises its stream once, which the events include), medians
over --reps; then the per-kernel times of one traced call.  Timings at a small
--n measure overheads.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_band_join import kernel_ms, run  # noqa: E402
from time_join_pairs import ROOT, alg_bytes, baseline_library, timed  # noqa: E402,F401


def outer_bytes(width, n_r, n_s, total):
    """Bytes an outer join into all five columns has to move: both passes
    read both relations, the write pass reads a tuple of each present side per
    row (at most 2 w) and writes two int64 and three value columns."""
    col = width // 2
    return 2 * (n_r + n_s) * width + total * (16 + 3 * col)


def finish(res, calls, args, torch, lib, traced):
    res.update(run(torch, calls, args.reps, args.warmup))
    res["outer_over_pairs"] = round(res["outer_full"]["median_ms"]
                                    / res["join_pairs"]["median_ms"], 3)
    res["alg_GBps"] = round(res["alg_GB"] * 1e3 / res["outer_full"]["median_ms"], 1)
    res["kernel_ms"] = {name: kernel_ms(torch, lib, calls[name]) for name in traced}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def sorted_inputs(torch, lib, n, s_total):
    """Sorted PK R (keys 1..n) and n tuples of the FK relation over 1..s_total"""
    R, S = lib.empty(n), lib.empty(n)
    lib.dev_gen_pk(R, 0, n, 12345)
    lib.dev_gen_fk(S, 0, s_total, s_total, 54321)
    sR, sS = lib.empty(n), lib.empty(n)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib.dev_join(R, S, sR, sS, cnt, 10, 1, s_total)
    pairs = int(cnt.item())
    del R, S
    torch.cuda.empty_cache()
    return sR, sS, pairs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--also", action="append", default=[], metavar="NAME=DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_join_timing.jsonl"))
    args = ap.parse_args()

    import torch
    import smj
    if not torch.cuda.is_available():
        sys.exit("time_outer_join: no HIP device (timings come from the GPU only)")
    n = args.n
    for width in args.widths:
        lib = smj.Library(width)
        others = {a.split("=", 1)[0]: baseline_library(smj, width, a.split("=", 1)[1])
                  for a in args.also}
        dt = torch.int32 if width == 8 else torch.int64
        base = {"width": width, "n": n, "reps": args.reps,
                "device": torch.cuda.get_device_name(0)}

        # covered: every key on both sides
        sR, sS, pairs = sorted_inputs(torch, lib, n, n)
        assert pairs == n, (pairs, n)
        oc = [torch.empty(n, dtype=dt, device="cuda") for _ in range(3)]
        pc = [torch.empty(n, dtype=dt, device="cuda") for _ in range(3)]
        out = lib.empty(n)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        calls = {
            "outer_full": lambda: lib.dev_outer_join(sR, sS, "full", None, None, *oc),
            "outer_inner": lambda: lib.dev_outer_join(sR, sS, "inner", None, None, *oc),
            "outer_full_count_only": lambda: lib.dev_outer_join(sR, sS, "full"),
            "outer_join_count": lambda: lib.dev_outer_join_count(sR, sS, "full", cnt),
            "join_pairs": lambda: lib.dev_join_pairs(sR, sS, *pc),
            "materialize": lambda: lib.dev_materialize(sR, sS, out),
        }
        for tag, o in others.items():
            calls["join_pairs_" + tag] = lambda o=o: o.dev_join_pairs(sR, sS, *pc)
            calls["materialize_" + tag] = lambda o=o: o.dev_materialize(sR, sS, out)
        for name, fn in calls.items():
            got = fn()
            assert got is None or got == n, (name, got, n)
        torch.cuda.synchronize()
        for a, b in zip(oc, pc):
            assert torch.equal(a, b), "outer join (full) and join pairs disagree"
        res = dict(base, part="covered", total=n, columns=["r_payload", "s_payload", "key"])
        b = alg_bytes(width, n, n, n, True)["join_pairs"]
        res["alg_GB"] = round(b / 1e9, 3)   # the join index's bytes
        finish(res, calls, args, torch, lib, ("outer_full", "join_pairs"))
        del sR, sS, oc, pc, out, calls
        torch.cuda.empty_cache()

        # half: about half of each side without a partner
        sR, sS, pairs = sorted_inputs(torch, lib, n, 2 * n)
        totals = {how: lib.dev_outer_join(sR, sS, how) for how in ("inner", "left", "right", "full")}
        assert totals["inner"] == pairs and totals["full"] == 2 * n - pairs, (totals, pairs)
        total = totals["full"]
        idx = [torch.empty(total, dtype=torch.int64, device="cuda") for _ in range(2)]
        val = [torch.empty(total, dtype=dt, device="cuda") for _ in range(3)]
        calls = {
            "outer_full": lambda: lib.dev_outer_join(sR, sS, "full", *idx, *val),
            "outer_left": lambda: lib.dev_outer_join(sR, sS, "left", *idx, *val),
            "outer_right": lambda: lib.dev_outer_join(sR, sS, "right", *idx, *val),
            "join_pairs": lambda: lib.dev_join_pairs(sR, sS, *[v[:pairs] for v in val]),
        }
        for name, fn in calls.items():
            fn()
        res = dict(base, part="half", pairs=pairs, totals=totals,
                   columns=["r_index", "s_index", "r_payload", "s_payload", "key"])
        b = outer_bytes(width, n, n, total)
        res["alg_GB"] = round(b / 1e9, 3)
        finish(res, calls, args, torch, lib, ("outer_full", "join_pairs"))
        del sR, sS, idx, val, calls
        torch.cuda.empty_cache()
        lib.reset_workspace()
        for o in others.values():
            o.reset_workspace()


if __name__ == "__main__":
    main()
