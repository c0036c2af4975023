#!/usr/bin/env python3
"""Time smj_dev_band_join on sorted PK R (keys 1..n) and FK S, in one process
(DESIGN.md §7's band-join numbers).

    python tools/time_band_join.py [--n 134217728] [--band-n 16777216]
                                   [--widths 16 8] [--reps 11] [--warmup 3]
                                   [--bands -1,1 -8,7] [--also NAME=DIR ...]

Per tuple width two lines of JSON are printed per part:

* band (0, 0) at --n tuples a side, beside smj_dev_join_pairs (with its key
  column; the band join writes the same three columns, r_key_out NULL) and
  smj_dev_merge_join_count, with the count-only forms; the ratios, and the
  per-kernel times of one traced call of each;
* each of --bands at --band-n tuples a side (the output of band (-8, 7) is
  16 pairs an S tuple: --band-n keeps its four columns within memory), beside
  smj_dev_join_pairs on the same inputs, with the output bytes per second of
  k_band_write and of k_pairs_write from their traced kernel times.

The calls run round-robin, each timed with device events (a call that
synchronises its stream is timed with that), medians over --reps.  --also
NAME=DIR names another build of the libraries (make BUILD=... LIBOUT=...):
its band join runs in the same round-robin as band_join_NAME.  Timings at a
small --n measure overheads.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_join_pairs import baseline_library, timed  # noqa: E402  (adds the package path)


def alg_bytes(width, n_r, n_s, total, ncols):
    """Bytes a band join of `total` pairs into ncols columns has to move."""
    col = width // 2
    count = (n_r + n_s) * width   # S tiles and their R windows, read
    ent = n_s * 8                 # (start, length) per S tuple, written then read
    write = (n_r + n_s) * width   # the R ranges and the S tuples, read again
    return count + 2 * ent + write + total * col * ncols


def kernel_ms(torch, lib, fn):
    lib.trace(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: round(v[0], 4) for k, v in lib.trace_read().items()}
    finally:
        lib.trace(False)


def run(torch, calls, reps, warmup):
    ms = {name: [] for name in calls}
    for it in range(warmup + reps):
        for name, fn in calls.items():
            t = timed(torch, fn)
            if it >= warmup:
                ms[name].append(t)
    return {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                   "max_ms": round(max(v), 4)} for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--band-n", type=int, default=1 << 24)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bands", nargs="*", default=["-1,1", "-8,7"], metavar="LO,HI")
    ap.add_argument("--also", action="append", default=[], metavar="NAME=DIR")
    args = ap.parse_args()

    import torch
    import smj
    if not torch.cuda.is_available():
        sys.exit("time_band_join: no HIP device (timings come from the GPU only)")
    bands = [tuple(int(x) for x in b.split(",")) for b in args.bands]
    for width in args.widths:
        lib = smj.Library(width)
        others = {a.split("=", 1)[0]: baseline_library(smj, width, a.split("=", 1)[1])
                  for a in args.also}
        dt = torch.int32 if width == 8 else torch.int64
        col = width // 2

        def relations(n):
            R, S = lib.empty(n), lib.empty(n)
            lib.dev_gen_pk(R, 0, n, 12345)
            lib.dev_gen_fk(S, 0, n, n, 54321)
            sR, sS = lib.empty(n), lib.empty(n)
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            lib.dev_join(R, S, sR, sS, cnt, 10, 1, n)
            return sR, sS, int(cnt.item())

        def columns(total, k):
            return [torch.empty(total, dtype=dt, device="cuda") for _ in range(k)]

        # ---- band (0, 0) beside the key join
        n = args.n
        sR, sS, total = relations(n)
        cols = columns(total, 4)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        three = (cols[0], cols[1], None, cols[2])
        calls = {
            "band_join": lambda: lib.dev_band_join(sR, sS, 0, 0, *three),
            "band_join_4col": lambda: lib.dev_band_join(sR, sS, 0, 0, *cols),
            "join_pairs": lambda: lib.dev_join_pairs(sR, sS, *cols[:3]),
            "band_count_only": lambda: lib.dev_band_join(sR, sS, 0, 0),
            "pairs_count_only": lambda: lib.dev_join_pairs(sR, sS),
            "band_join_count": lambda: lib.dev_band_join_count(sR, sS, 0, 0, cnt),
            "merge_join_count": lambda: lib.dev_merge_join_count(sR, sS, cnt),
        }
        for tag, o in others.items():
            calls["band_join_" + tag] = lambda o=o: o.dev_band_join(sR, sS, 0, 0, *three)
        for name, fn in calls.items():
            got = fn()
            assert got is None or got == total, (name, got, total)
        res = {"part": "band00", "width": width, "n": n, "total": total, "reps": args.reps,
               "device": torch.cuda.get_device_name(0)}
        res.update(run(torch, calls, args.reps, args.warmup))
        b3 = alg_bytes(width, n, n, total, 3)
        res["band_join"]["alg_GB"] = round(b3 / 1e9, 3)
        res["band_join"]["alg_GBps"] = round(b3 / res["band_join"]["median_ms"] / 1e6, 1)
        res["band_over_pairs"] = round(res["band_join"]["median_ms"]
                                       / res["join_pairs"]["median_ms"], 3)
        res["band_count_over_merge_count"] = round(res["band_join_count"]["median_ms"]
                                                   / res["merge_join_count"]["median_ms"], 3)
        res["kernel_ms"] = {name: kernel_ms(torch, lib, calls[name])
                            for name in ("band_join", "join_pairs")}
        for tag, o in others.items():
            res["kernel_ms"]["band_join_" + tag] = kernel_ms(torch, o, calls["band_join_" + tag])
        print(json.dumps(res), flush=True)
        del sR, sS, cols, three, calls
        torch.cuda.empty_cache()

        # ---- wider bands: the write pass's output rate
        n = args.band_n
        if bands:
            sR, sS, key_total = relations(n)
            pcols = columns(key_total, 3)
        for lo, hi in bands:
            total = lib.dev_band_join(sR, sS, lo, hi)
            cols = columns(total, 4)
            calls = {
                "band_join": lambda: lib.dev_band_join(sR, sS, lo, hi, *cols),
                "join_pairs": lambda: lib.dev_join_pairs(sR, sS, *pcols),
            }
            for tag, o in others.items():
                calls["band_join_" + tag] = lambda o=o: o.dev_band_join(sR, sS, lo, hi, *cols)
            for name, fn in calls.items():
                got = fn()
                assert got == (key_total if name == "join_pairs" else total), (name, got)
            res = {"part": "band", "band": [lo, hi], "width": width, "n": n, "total": total,
                   "key_join_total": key_total, "output_GB": round(total * 4 * col / 1e9, 3),
                   "note": f"n = {n} a side keeps four output columns of band (-8, 7) "
                           "(16 pairs an S tuple) within memory",
                   "reps": args.reps, "device": torch.cuda.get_device_name(0)}
            res.update(run(torch, calls, args.reps, args.warmup))
            b4 = alg_bytes(width, n, n, total, 4)
            res["band_join"]["alg_GB"] = round(b4 / 1e9, 3)
            res["band_join"]["alg_GBps"] = round(b4 / res["band_join"]["median_ms"] / 1e6, 1)
            km = {name: kernel_ms(torch, lib, calls[name]) for name in ("band_join", "join_pairs")}
            for tag, o in others.items():
                km["band_join_" + tag] = kernel_ms(torch, o, calls["band_join_" + tag])
            res["kernel_ms"] = km
            # output bytes per second of the two write kernels, from their own times
            res["k_band_write_out_GBps"] = round(
                total * 4 * col / km["band_join"]["k_band_write"] / 1e6, 1)
            res["k_pairs_write_out_GBps"] = round(
                key_total * 3 * col / km["join_pairs"]["k_pairs_write"] / 1e6, 1)
            for tag in others:
                res[f"k_band_write_{tag}_out_GBps"] = round(
                    total * 4 * col / km["band_join_" + tag]["k_band_write"] / 1e6, 1)
            print(json.dumps(res), flush=True)
            del cols, calls
            torch.cuda.empty_cache()
        lib.reset_workspace()
        for o in others.values():
            o.reset_workspace()


if __name__ == "__main__":
    main()
