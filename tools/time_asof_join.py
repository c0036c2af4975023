#!/usr/bin/env python3
"""Time smj_dev_asof_join on sorted PK R (keys 1..n) and FK S, in one process
(DESIGN.md §7's as-of join numbers).

    python tools/time_asof_join.py [--n 134217728] [--widths 16 8] [--reps 11]
                                   [--warmup 3] [--out profiles/asof_join_timing.jsonl]

Per tuple width one line of JSON is printed and appended to --out: the as-of
join writing two columns (r_index, r_payload) backward, forward, nearest, and
backward with groups of 2^16 keys and a tolerance of 4, beside
smj_dev_band_join at band (0, 0) writing its two payload columns and
smj_dev_band_join_count at (0, 0) on the same inputs; the ratio of the
backward as-of join to the band join; the per-kernel times of one traced call
of each; and the bytes the as-of join has to move, (nR + nS) * width read
plus the columns written.

The calls run round-robin, each timed with device events (the band join
synchronises its stream once and is timed with that), medians over --reps.
Timings at a small --n measure overheads.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_band_join import kernel_ms, run  # noqa: E402
from time_join_pairs import ROOT, timed  # noqa: E402,F401  (adds the package path; run() times with it)

GROUP_SHIFT, TOLERANCE = 16, 4


def alg_bytes(width, n_r, n_s):
    """Bytes an as-of join into r_index and r_payload has to move."""
    return (n_r + n_s) * width + n_s * (8 + width // 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asof_join_timing.jsonl"))
    args = ap.parse_args()

    import torch
    import smj
    if not torch.cuda.is_available():
        sys.exit("time_asof_join: no HIP device (timings come from the GPU only)")
    for width in args.widths:
        lib = smj.Library(width)
        dt = torch.int32 if width == 8 else torch.int64
        n = args.n
        R, S = lib.empty(n), lib.empty(n)
        lib.dev_gen_pk(R, 0, n, 12345)
        lib.dev_gen_fk(S, 0, n, n, 54321)
        sR, sS = lib.empty(n), lib.empty(n)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        lib.dev_join(R, S, sR, sS, cnt, 10, 1, n)
        total = int(cnt.item())
        del R, S
        torch.cuda.empty_cache()
        idx = torch.empty(n, dtype=torch.int64, device="cuda")
        pay = torch.empty(n, dtype=dt, device="cuda")
        br, bs = (torch.empty(total, dtype=dt, device="cuda") for _ in range(2))
        calls = {
            "asof_backward": lambda: lib.dev_asof_join(sR, sS, "backward", False, None, 0,
                                                       idx, pay),
            "asof_forward": lambda: lib.dev_asof_join(sR, sS, "forward", False, None, 0,
                                                      idx, pay),
            "asof_nearest": lambda: lib.dev_asof_join(sR, sS, "nearest", False, None, 0,
                                                      idx, pay),
            "asof_backward_groups_tol": lambda: lib.dev_asof_join(
                sR, sS, "backward", False, TOLERANCE, GROUP_SHIFT, idx, pay),
            "band_join": lambda: lib.dev_band_join(sR, sS, 0, 0, br, bs),
            "band_join_count": lambda: lib.dev_band_join_count(sR, sS, 0, 0, cnt),
        }
        # every S key of the FK relation occurs in the PK relation: all rows
        # match at distance 0, and the band join (0, 0) has one pair a row
        assert total == n, (total, n)
        for name, fn in calls.items():
            got = fn()
            assert got is None or got == total, (name, got, total)
        torch.cuda.synchronize()
        assert int((idx < 0).sum().item()) == 0
        assert torch.equal(pay, br), "as-of backward with groups and band (0, 0) disagree"
        res = {"part": "asof", "width": width, "n": n, "band_total": total, "reps": args.reps,
               "columns": ["r_index", "r_payload"], "group_shift": GROUP_SHIFT,
               "tolerance": TOLERANCE, "device": torch.cuda.get_device_name(0)}
        res.update(run(torch, calls, args.reps, args.warmup))
        b = alg_bytes(width, n, n)
        for name in calls:
            if name.startswith("asof_"):
                res[name]["alg_GB"] = round(b / 1e9, 3)
                res[name]["alg_GBps"] = round(b / res[name]["median_ms"] / 1e6, 1)
        res["asof_over_band"] = round(res["asof_backward"]["median_ms"]
                                      / res["band_join"]["median_ms"], 3)
        res["kernel_ms"] = {name: kernel_ms(torch, lib, calls[name])
                            for name in ("asof_backward", "asof_nearest", "band_join")}
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del sR, sS, idx, pay, br, bs, calls
        torch.cuda.empty_cache()
        lib.reset_workspace()


if __name__ == "__main__":
    main()
