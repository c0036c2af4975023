#!/usr/bin/env python3
"""Time smj_dev_group_aggregate on sorted relations, in one process (DESIGN.md
§7's group-aggregate numbers).

    python tools/time_group_aggregate.py [--n 134217728] [--widths 16 8] [--reps 11]
                                         [--warmup 3] [--fk-dup 4]
                                         [--out profiles/group_aggregate_timing.jsonl]

Per tuple width one line of JSON is printed and appended to --out: the call
writing three columns (key, count, sum) on

* pk         the sorted PK relation (keys 1..n: every tuple a head, n groups);
* fk         the sorted uniform FK relation (keys 1..n / --fk-dup, each
             --fk-dup times);
* fk_shift16 the same with group_shift = 16 (runs crossing many tiles);
* hot        one key (all keys equal: one group over every tile);

each beside torch.unique_consecutive(keys, return_counts=True) on the
contiguous key column of the same sorted relation (for fk_shift16 the column
key >> 16, prepared outside the timed region).  That baseline yields keys and
counts only, so it does strictly less.  Per call: median, min and max over
--reps, the per-kernel times of one traced call, the bytes the call has to
move (n * width read once plus the rows written; the kernels read the
relation twice, so the rate against these bytes stays below the copy rate)
and the rate; per input the ratio torch / library.

The calls run round-robin, each timed with device events (the library call
synchronises its stream once and is timed with that).  Timings at a small
--n measure overheads.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_band_join import kernel_ms, run  # noqa: E402
from time_join_pairs import ROOT  # noqa: E402,F401  (adds the package path)

GROUP_SHIFT = 16


def alg_bytes(width, n, rows):
    """Bytes a call into key, count and sum has to move."""
    return n * width + rows * (width // 2 + 8 + 8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fk-dup", type=int, default=4)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "group_aggregate_timing.jsonl"))
    args = ap.parse_args()

    import torch
    import smj
    if not torch.cuda.is_available():
        sys.exit("time_group_aggregate: no HIP device (timings come from the GPU only)")
    for width in args.widths:
        lib = smj.Library(width)
        dt = torch.int32 if width == 8 else torch.int64
        n = args.n
        maxid = max(n // args.fk_dup, 1)
        tmp = lib.empty(n)
        pk, fk = lib.empty(n), lib.empty(n)
        lib.dev_gen_pk(tmp, 0, n, 12345)
        lib.dev_sort(tmp, pk)
        lib.dev_gen_fk(tmp, 0, n, maxid, 54321)
        lib.dev_sort(tmp, fk)
        hot = tmp
        hot.copy_(fk)
        hot[:, 1] = 7
        torch.cuda.synchronize()
        inputs = {"pk": (pk, 0), "fk": (fk, 0), "fk_shift16": (fk, GROUP_SHIFT), "hot": (hot, 0)}
        keys = {name: (t[:, 1] >> sh).contiguous() for name, (t, sh) in inputs.items()}
        groups = {name: lib.dev_group_aggregate(t, sh) for name, (t, sh) in inputs.items()}
        assert groups["pk"] == n and groups["hot"] == 1, groups
        cap = max(groups.values())
        key = torch.empty(cap, dtype=dt, device="cuda")
        count, total = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(2))
        calls = {}
        for name, (t, sh) in inputs.items():
            calls[name] = lambda t=t, sh=sh: lib.dev_group_aggregate(
                t, sh, key=key, count=count, sum=total)
            calls["torch_" + name] = lambda k=keys[name]: torch.unique_consecutive(
                k, return_counts=True)
        # the two agree on what they both give
        for name, (t, sh) in inputs.items():
            assert calls[name]() == groups[name], name
            uk, uc = calls["torch_" + name]()
            g = groups[name]
            assert uk.shape[0] == g and torch.equal(uc, count[:g]), name
            assert torch.equal(uk, key[:g] >> sh), name
            assert int(total[:g].sum().item()) == int(t[:, 0].sum().item()), name
            del uk, uc
        res = {"part": "group_aggregate", "width": width, "n": n, "reps": args.reps,
               "columns": ["key", "count", "sum"], "fk_maxid": maxid,
               "group_shift": GROUP_SHIFT, "tile": lib.group_tile(), "groups": groups,
               "device": torch.cuda.get_device_name(0)}
        res.update(run(torch, calls, args.reps, args.warmup))
        res["torch_over_library"] = {}
        res["kernel_ms"] = {}
        for name in inputs:
            b = alg_bytes(width, n, groups[name])
            res[name]["alg_GB"] = round(b / 1e9, 3)
            res[name]["alg_GBps"] = round(b / res[name]["median_ms"] / 1e6, 1)
            res["torch_over_library"][name] = round(
                res["torch_" + name]["median_ms"] / res[name]["median_ms"], 3)
            res["kernel_ms"][name] = kernel_ms(torch, lib, calls[name])
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del pk, fk, hot, tmp, inputs, keys, key, count, total, calls
        torch.cuda.empty_cache()
        lib.reset_workspace()


if __name__ == "__main__":
    main()
