#!/usr/bin/env python3
"""Time smj_dev_materialize, smj_dev_join_pairs and smj_dev_semi_join on the
same sorted inputs, in one process (DESIGN.md §7's join-index numbers).

    python tools/time_join_pairs.py [--n 134217728] [--widths 16 8]
                                    [--reps 11] [--warmup 3] [--trace]
                                    [--also NAME=DIR ...]

Per tuple width and workload (PK/FK, and a Zipf-0.75 S against the same PK R)
the relations are generated and joined on the device once; the three calls
then run round-robin on the sorted relations, each timed with device events
(every call synchronises its stream once, which the events include), and the
medians are printed as one JSON line.  --also NAME=DIR names another build
of the libraries (make BUILD=... LIBOUT=...): its smj_dev_materialize, and
its smj_dev_join_pairs and smj_dev_semi_join where it has them, join the
round-robin as materialize_NAME / join_pairs_NAME / semi_join_NAME, so an older
commit's kernels or a variant
build are timed beside this one's.
--trace adds the per-kernel times of one more join-pairs call.  --n shrinks
the relations for a functional check; timings at small n measure overheads.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "avx-sort-merge-joins_amd"))


def baseline_library(smj, width, libdir):
    name = os.path.basename(smj.lib_path(width))
    # an older build may lack newer entry points: the binding leaves those
    # unbound only for a library selected through SMJ_LIB_DIR
    old = os.environ.get("SMJ_LIB_DIR")
    os.environ["SMJ_LIB_DIR"] = libdir
    try:
        return smj.Library(width, path=os.path.join(libdir, name))
    finally:
        if old is None:
            del os.environ["SMJ_LIB_DIR"]
        else:
            os.environ["SMJ_LIB_DIR"] = old


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alg_bytes(width, n_r, n_s, total, with_keys):
    """Bytes each call has to move for a key join of `total` matches."""
    col = width // 2
    count = (n_r + n_s) * width           # S tiles and their R windows, read
    mat = count + n_s * width + total * width
    pairs = (count + n_s * 4               # partner offsets written
             + n_s * (width + 4)           # S and the offsets read again
             + total * col                 # gathered R payloads (of 32-B sectors more)
             + total * col * (3 if with_keys else 2))
    semi = count + n_s * width + total * width
    return {"materialize": mat, "join_pairs": pairs, "semi_join": semi}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-keys", action="store_true", help="join pairs without the key column")
    ap.add_argument("--also", action="append", default=[], metavar="NAME=DIR")
    args = ap.parse_args()

    import torch
    import smj
    if not torch.cuda.is_available():
        sys.exit("time_join_pairs: no HIP device (timings come from the GPU only)")
    n = args.n
    for width in args.widths:
        lib = smj.Library(width)
        others = {a.split("=", 1)[0]: baseline_library(smj, width, a.split("=", 1)[1])
                  for a in args.also}
        dt = torch.int32 if width == 8 else torch.int64
        for workload in ("pkfk", "zipf0.75"):
            R, S = lib.empty(n), lib.empty(n)
            lib.dev_gen_pk(R, 0, n, 12345)
            if workload == "pkfk":
                lib.dev_gen_fk(S, 0, n, n, 54321)
            else:
                lib.dev_gen_zipf(S, 0, n, 0.75, 54321)
            sR, sS = lib.empty(n), lib.empty(n)
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            lib.dev_join(R, S, sR, sS, cnt, 10, 1, n)
            total = int(cnt.item())
            del R, S
            out = lib.empty(total)
            cols = [torch.empty(total, dtype=dt, device="cuda")
                    for _ in range(2 if args.no_keys else 3)]
            calls = {
                "materialize": lambda: lib.dev_materialize(sR, sS, out),
                "join_pairs": lambda: lib.dev_join_pairs(sR, sS, *cols),
                "semi_join": lambda: lib.dev_semi_join(sR, sS, out),
            }
            for tag, o in others.items():
                calls["materialize_" + tag] = lambda o=o: o.dev_materialize(sR, sS, out)
                if hasattr(o.lib, "smj_dev_join_pairs"):
                    calls["join_pairs_" + tag] = lambda o=o: o.dev_join_pairs(sR, sS, *cols)
                if hasattr(o.lib, "smj_dev_semi_join"):
                    calls["semi_join_" + tag] = lambda o=o: o.dev_semi_join(sR, sS, out)
            for name, fn in calls.items():
                got = fn()
                assert got == total, (name, got, total)
            ms = {name: [] for name in calls}
            for it in range(args.warmup + args.reps):
                for name, fn in calls.items():
                    t = timed(torch, fn)
                    if it >= args.warmup:
                        ms[name].append(t)
            res = {"width": width, "workload": workload, "n": n, "total": total,
                   "reps": args.reps, "device": torch.cuda.get_device_name(0)}
            bytes_ = alg_bytes(width, n, n, total, not args.no_keys)
            for name, v in ms.items():
                med = statistics.median(v)
                res[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                             "max_ms": round(max(v), 4)}
                b = bytes_[next(k for k in bytes_ if name.startswith(k))]
                res[name]["alg_GB"] = round(b / 1e9, 3)
                res[name]["alg_GBps"] = round(b / med / 1e6, 1)
            m = res["materialize"]["median_ms"]
            res["pairs_over_materialize"] = round(res["join_pairs"]["median_ms"] / m, 3)
            res["semi_over_materialize"] = round(res["semi_join"]["median_ms"] / m, 3)
            if args.trace:
                res["kernel_ms"] = {}
                for name in ("materialize", "join_pairs", "semi_join"):
                    lib.trace(True)
                    calls[name]()
                    torch.cuda.synchronize()
                    res["kernel_ms"][name] = {k: round(v[0], 4)
                                              for k, v in lib.trace_read().items()}
                    lib.trace(False)
            print(json.dumps(res), flush=True)
            del sR, sS, out, cols, calls
            torch.cuda.empty_cache()
        lib.reset_workspace()
        for o in others.values():
            o.reset_workspace()


if __name__ == "__main__":
    main()
