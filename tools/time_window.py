#!/usr/bin/env python3
"""Time smj_dev_window on sorted relations, in one process (DESIGN.md §7's
window numbers).

    python tools/time_window.py [--n 134217728] [--widths 16 8] [--reps 11]
                                [--warmup 3] [--fk-dup 4]
                                [--out profiles/window_timing.jsonl]

Per tuple width one line of JSON is printed and appended to --out.  The inputs
are tools/time_group_aggregate.py's:

* pk         the sorted PK relation (keys 1..n: every tuple a head, n groups);
* fk         the sorted uniform FK relation (keys 1..n / --fk-dup, each
             --fk-dup times);
* fk_shift16 the same with group_shift = 16 (runs crossing many tiles, and
             the only input on which rank and dense_rank are not all 0);
* hot        one key (all keys equal: one group over every tile).

On each, two forms of the call: `<input>` writes (row, sum), `<input>_all` all
seven columns.  Beside them, in the same round-robin:

* torch_<input>  torch.cumsum of the contiguous payload column of the same
                 relation (prepared outside the timed region).  It is
                 unsegmented and reads 8 or 4 bytes a tuple once, so it does
                 strictly less;
* group_<input>  dev_group_aggregate(key, count, sum) on the same input.

Per call: median, min and max over --reps, the per-kernel times of one traced
call, the bytes the call has to move (n * width read once plus n times the
bytes of the columns written; the kernels read the relation twice, so the rate
against these bytes stays below the copy rate) and the rate; for the write
pass alone its physical bytes (the same sum: it reads the relation once) and
their rate; per input the ratio torch / library of both forms.

The calls run round-robin, each timed with device events (the window call does
not synchronise; the group aggregate synchronises its stream once and is timed
with that).  Timings at a small --n measure overheads.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_band_join import kernel_ms, run  # noqa: E402
from time_join_pairs import ROOT  # noqa: E402,F401  (adds the package path)

GROUP_SHIFT = 16
FORMS = {"": ("row", "sum"),
         "_all": ("group", "row", "rank", "dense_rank", "sum", "min", "max")}


def alg_bytes(width, n, columns):
    """Bytes a call into `columns` has to move."""
    return n * width + n * sum(width // 2 if c in ("min", "max") else 8 for c in columns)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fk-dup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_timing.jsonl"))
    args = ap.parse_args()

    import torch
    import smj
    if not torch.cuda.is_available():
        sys.exit("time_window: no HIP device (timings come from the GPU only)")
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
        pays = {name: t[:, 0].contiguous() for name, (t, sh) in inputs.items()}
        groups = {name: lib.dev_group_aggregate(t, sh) for name, (t, sh) in inputs.items()}
        assert groups["pk"] == n and groups["hot"] == 1, groups
        cols = {c: torch.empty(n, dtype=dt if c in ("min", "max") else torch.int64, device="cuda")
                for c in FORMS["_all"]}
        cap = max(groups.values())
        gkey = torch.empty(cap, dtype=dt, device="cuda")
        gcount, gsum = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(2))
        calls = {}
        for name, (t, sh) in inputs.items():
            for form, which in FORMS.items():
                calls[name + form] = lambda t=t, sh=sh, which=which: lib.dev_window(
                    t, sh, **{c: cols[c] for c in which})
            calls["torch_" + name] = lambda p=pays[name]: torch.cumsum(p, 0)
            calls["group_" + name] = lambda t=t, sh=sh: lib.dev_group_aggregate(
                t, sh, key=gkey, count=gcount, sum=gsum)
        # what the calls must agree on: one group is the unsegmented cumsum,
        # all heads give the payloads back, and the group table's rows are the
        # window's values at each group's last tuple
        for name, (t, sh) in inputs.items():
            cols["sum"].fill_(-1)
            calls[name]()
            two = cols["sum"].clone()
            calls[name + "_all"]()
            assert torch.equal(two, cols["sum"]), name
            del two
            g = calls["group_" + name]()
            last = torch.cumsum(gcount[:g], 0) - 1
            assert torch.equal(cols["sum"][last], gsum[:g]), name
            assert torch.equal(cols["row"][last] + 1, gcount[:g]), name
            assert int(cols["group"][-1].item()) == g - 1, name
            if name == "hot":
                assert torch.equal(cols["sum"], calls["torch_hot"]()), name
            if name == "pk":
                assert torch.equal(cols["sum"], pays[name].to(torch.int64)), name
                assert not bool(cols["row"].any()), name
            assert bool(cols["dense_rank"].any()) == (name == "fk_shift16"), name
            del last
        res = {"part": "window", "width": width, "n": n, "reps": args.reps,
               "forms": {k or "two": list(v) for k, v in FORMS.items()}, "fk_maxid": maxid,
               "group_shift": GROUP_SHIFT, "tile": lib.window_tile(), "groups": groups,
               "device": torch.cuda.get_device_name(0)}
        res.update(run(torch, calls, args.reps, args.warmup))
        res["torch_over_library"] = {}
        res["kernel_ms"] = {}
        for name in inputs:
            for form, which in FORMS.items():
                r = res[name + form]
                b = alg_bytes(width, n, which)
                r["alg_GB"] = round(b / 1e9, 3)
                r["alg_GBps"] = round(b / r["median_ms"] / 1e6, 1)
                k = kernel_ms(torch, lib, calls[name + form])
                res["kernel_ms"][name + form] = k
                r["write_GBps"] = round(b / k["k_window_write"] / 1e6, 1)
                res["torch_over_library"][name + form] = round(
                    res["torch_" + name]["median_ms"] / r["median_ms"], 3)
            res["kernel_ms"]["group_" + name] = kernel_ms(torch, lib, calls["group_" + name])
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del pk, fk, hot, tmp, inputs, pays, cols, gkey, gcount, gsum, calls
        torch.cuda.empty_cache()
        lib.reset_workspace()


if __name__ == "__main__":
    main()
