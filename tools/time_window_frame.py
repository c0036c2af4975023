#!/usr/bin/env python3
"""Time smj_dev_window_frame on sorted relations, in one process (DESIGN.md
§7's window-frame numbers).

    python tools/time_window_frame.py [--n 134217728] [--widths 16 8] [--reps 11]
                                      [--warmup 3] [--fk-dup 4]
                                      [--out profiles/window_frame_timing.jsonl]

Per tuple width one line of JSON is printed and appended to --out.  The inputs
are three of tools/time_window.py's:

* fk         the sorted uniform FK relation (keys 1..n / --fk-dup, each
             --fk-dup times);
* fk_shift16 the same with group_shift = 16 (groups crossing many tiles);
* hot        one key (all keys equal: one group over every tile).

On each, the forms of FORMS below: `<input>/<form>`.  Beside them, in the same
round-robin:

* `<input>/window_sum`, `<input>/window_agg`  dev_window into the same columns
  (sum; sum, min, max) on the same input: it computes the same values as the
  forms rows_run_sum and rows_run_agg;
* `<input>/torch_roll100`  torch.cumsum of the contiguous payload column and a
  shifted difference, the unsegmented rolling sum of width 100: it does
  strictly less than rows_w100_all.

Per call: median, min and max over --reps, the per-kernel times of one traced
call, the algorithmic bytes (the relation once plus the columns written) and
the rate against them, and the bytes of per-element workspace tables the build
pass writes and the write pass looks up (two entries a row and table), the
relation's second read, and the rate with all of them.  Before timing the
tool asserts on its own inputs what ties the frames to dev_window, to the group
table and to each other.

The calls run round-robin, each timed with device events (no call
synchronises).  Timings at a small --n measure overheads.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_band_join import kernel_ms, run  # noqa: E402
from time_join_pairs import ROOT  # noqa: E402,F401  (adds the package path)

GROUP_SHIFT = 16
ALL = ("start", "count", "sum", "min", "max", "first", "last")
# form -> (unit, lo, hi, columns); None is unbounded
FORMS = {
    "rows_run_sum": ("rows", None, 0, ("sum",)),
    "rows_run_agg": ("rows", None, 0, ("sum", "min", "max")),
    "rows_w100_all": ("rows", -99, 0, ALL),
    "rows_lag1": ("rows", -1, -1, ("first",)),
    "range_run_sum": ("range", None, 0, ("sum",)),
    "range_w60_all": ("range", -60, 0, ALL),
    "rows_total_sum": ("rows", None, None, ("sum",)),
}
WINDOW = {"window_sum": ("sum",), "window_agg": ("sum", "min", "max")}


def col_bytes(width, c):
    return 8 if c in ("start", "count", "sum", "group", "row") else width // 2


def alg_bytes(width, n, columns):
    """Bytes a call into `columns` has to move."""
    return n * width + n * sum(col_bytes(width, c) for c in columns)


def table_bytes(width, n, columns):
    """(written, read) bytes of the per-element tables of a frame call: the
    build pass writes the prefix sum (8 bytes a row) and, per extreme, its
    prefix and suffix in the block (two value_t a row); the write pass looks
    up two entries a row in each: the prefix sums at both ends of the frame,
    the suffix at its start and the prefix at its end."""
    ext = sum(width for c in ("min", "max") if c in columns)
    has_sum = "sum" in columns
    return n * (8 * has_sum + ext), n * (16 * has_sum + ext)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fk-dup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_frame_timing.jsonl"))
    args = ap.parse_args()

    import torch
    import smj
    if not torch.cuda.is_available():
        sys.exit("time_window_frame: no HIP device (timings come from the GPU only)")
    for width in args.widths:
        lib = smj.Library(width)
        dt = torch.int32 if width == 8 else torch.int64
        n = args.n
        maxid = max(n // args.fk_dup, 1)
        tmp, fk = lib.empty(n), lib.empty(n)
        lib.dev_gen_fk(tmp, 0, n, maxid, 54321)
        lib.dev_sort(tmp, fk)
        hot = tmp
        hot.copy_(fk)
        hot[:, 1] = 7
        torch.cuda.synchronize()
        inputs = {"fk": (fk, 0), "fk_shift16": (fk, GROUP_SHIFT), "hot": (hot, 0)}
        pays = {name: t[:, 0].contiguous() for name, (t, sh) in inputs.items()}
        cols = {c: torch.empty(n, dtype=torch.int64 if c in ("start", "count", "sum") else dt,
                               device="cuda") for c in ALL}
        wcols = {c: torch.empty(n, dtype=torch.int64 if c in ("group", "row", "sum") else dt,
                                device="cuda") for c in ("group", "row", "sum", "min", "max")}

        def frame(t, sh, form, into=cols):
            unit, lo, hi, which = FORMS[form]
            lib.dev_window_frame(t, sh, unit, lo, hi, **{c: into[c] for c in which})

        def roll100(p):
            c = torch.cumsum(p, 0)
            out = c.clone()
            out[100:] -= c[:-100]
            return out

        calls = {}
        for name, (t, sh) in inputs.items():
            for form in FORMS:
                calls[f"{name}/{form}"] = lambda t=t, sh=sh, form=form: frame(t, sh, form)
            for form, which in WINDOW.items():
                calls[f"{name}/{form}"] = lambda t=t, sh=sh, which=which: lib.dev_window(
                    t, sh, **{c: wcols[c] for c in which})
            calls[f"{name}/torch_roll100"] = lambda p=pays[name]: roll100(p)

        # what the calls must agree on
        for name, (t, sh) in inputs.items():
            lib.dev_window(t, sh, **wcols)
            frame(t, sh, "rows_run_agg")
            lib.dev_window_frame(t, sh, "rows", None, 0, start=cols["start"], count=cols["count"])
            for c in ("sum", "min", "max"):
                assert torch.equal(cols[c], wcols[c]), (name, c)
            assert torch.equal(cols["count"], wcols["row"] + 1), name
            run_sum = cols["sum"].clone()
            frame(t, sh, "rows_run_sum")
            assert torch.equal(cols["sum"], run_sum), name
            # the group's total per tuple is the group table gathered by the group column
            groups = lib.dev_group_aggregate(t, sh)
            gsum = torch.empty(groups, dtype=torch.int64, device="cuda")
            assert lib.dev_group_aggregate(t, sh, sum=gsum) == groups
            frame(t, sh, "rows_total_sum")
            assert torch.equal(cols["sum"], gsum[wcols["group"]]), name
            del gsum
            # RANGE (0, 0) counts the key run; RANGE (-inf, 0) is ROWS (-inf, 0) at the
            # row's last peer
            lib.dev_window_frame(t, sh, "range", 0, 0, start=cols["start"], count=cols["count"])
            keys = t[:, 1].contiguous()
            _, runs = torch.unique_consecutive(keys, return_counts=True)
            assert torch.equal(cols["count"], torch.repeat_interleave(runs, runs)), name
            last_peer = cols["start"] + cols["count"] - 1
            frame(t, sh, "range_run_sum")
            assert torch.equal(cols["sum"], run_sum[last_peer]), name
            # the width-100 sum inside one group is the unsegmented one
            if name == "hot":
                frame(t, sh, "rows_w100_all")
                assert torch.equal(cols["sum"], roll100(pays[name]).to(torch.int64)), name
                assert int(cols["count"][-1].item()) == min(n, 100), name
            del keys, runs, last_peer, run_sum
        res = {"part": "window_frame", "width": width, "n": n, "reps": args.reps,
               "forms": {k: [v[0], v[1], v[2], list(v[3])] for k, v in FORMS.items()},
               "window_forms": {k: list(v) for k, v in WINDOW.items()}, "fk_maxid": maxid,
               "group_shift": GROUP_SHIFT, "tile": lib.frame_tile(), "block": lib.frame_block(),
               "device": torch.cuda.get_device_name(0)}
        res.update(run(torch, calls, args.reps, args.warmup))
        res["kernel_ms"] = {}
        res["frame_over_window"] = {}
        for name in inputs:
            for form, which in list((f, v[3]) for f, v in FORMS.items()) + list(WINDOW.items()):
                r = res[f"{name}/{form}"]
                b = alg_bytes(width, n, which)
                r["alg_GB"] = round(b / 1e9, 3)
                r["alg_GBps"] = round(b / r["median_ms"] / 1e6, 1)
                res["kernel_ms"][f"{name}/{form}"] = kernel_ms(torch, lib, calls[f"{name}/{form}"])
                if form in FORMS:
                    wr, rd = table_bytes(width, n, which)
                    # the relation is read by the build (or heads) pass and by the write pass
                    phys = b + n * width + wr + rd
                    r["table_write_GB"] = round(wr / 1e9, 3)
                    r["table_read_GB"] = round(rd / 1e9, 3)
                    r["phys_GBps"] = round(phys / r["median_ms"] / 1e6, 1)
            for form, wform in (("rows_run_sum", "window_sum"), ("rows_run_agg", "window_agg")):
                res["frame_over_window"][f"{name}/{form}"] = round(
                    res[f"{name}/{form}"]["median_ms"] / res[f"{name}/{wform}"]["median_ms"], 3)
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del fk, hot, tmp, inputs, pays, cols, wcols, calls
        torch.cuda.empty_cache()
        lib.reset_workspace()


if __name__ == "__main__":
    main()
