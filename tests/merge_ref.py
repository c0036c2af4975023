"""Expected values of the merges (csrc/mergesort.hip), a restatement of the host
decision of the k-way merge, and the table of cases the GPU test runs: a
helper of test_merge_cases.py and test_gpu_merge_edges.py.

Reference.  The output of any merge is the sorted concatenation of its inputs
under the tuple order: at 8 bytes the signed int64 order of the packed word
key << 32 | uint32(payload) (so within a key negative payloads sort above the
others), at 16 bytes np.lexsort((payload, key)).  Fully equal tuples cannot be
told apart, so that is the one answer; nothing is said about the order of ties
between inputs.  loop_merge is heapq.merge on tuples of Python integers.  The
join count is sum_k |R_k| |S_k| from np.unique in Python integers.

decide() restates multiway_merge_buckets: the form, the bucket bits D, the bit
length L of the key range, the bucket shift s, every bucket's total and the
buckets larger than KM_CAP, which k_km_merge queues for k_km_over.  A case
states its promise in these terms; test_merge_cases.py checks each promise on
the CPU and test_gpu_merge_edges.py asserts the library's own record
(smj_workspace_merge_stats) against it in front of every comparison.
"""
import heapq

import numpy as np

from test_gpu_parity import rand_tuples

# the geometry of the kernels (csrc/mergesort.hip)
MG_TILE = 2048     # outputs of one workgroup of k_mergetile
KM_KMAX = 256      # most runs of the one-pass merge
KM_LOGNB = 12      # digit bits k_km_merge sorts in LDS
KM_RUNMAX = 64     # longest equal-digit run it fixes serially
MJ_GRID = 4096 * 256   # threads of k_mjcount's largest grid
SENTINEL = 0x5A5A5A5A  # placement.SENTINEL: (SENTINEL, SENTINEL) is in no input

DT = {8: np.dtype([("payload", "<i4"), ("key", "<i4")]),
      16: np.dtype([("payload", "<i8"), ("key", "<i8")])}


def cap(width):
    """KM_CAP: the tuples of a bucket that fit k_km_merge's LDS buffer."""
    return 4096 if width == 8 else 2048


def limits(width):
    """The smallest and largest key (and payload) of the width."""
    return (-(1 << 31), (1 << 31) - 1) if width == 8 else (-(1 << 63), (1 << 63) - 1)


def tup(width, keys, payloads):
    keys = np.asarray(keys, np.int64)
    t = np.zeros(len(keys), DT[width])
    t["key"] = keys
    t["payload"] = payloads
    return t


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def order_of(t):
    """The permutation that sorts the structured array t in the tuple order."""
    if t.dtype.itemsize == 8:
        w = (t["key"].astype(np.int64) << 32) | (t["payload"].astype(np.int64) & 0xFFFFFFFF)
        return np.argsort(w, kind="stable")
    return np.lexsort((t["payload"], t["key"]))


def srt(t):
    return t[order_of(t)]


def numpy_merge(runs, width):
    runs = [r for r in runs if len(r)]
    if not runs:
        return np.zeros(0, DT[width])
    return srt(np.concatenate(runs))


def _pytuples(t):
    if t.dtype.itemsize == 8:
        return [(k, p & 0xFFFFFFFF, p) for k, p in zip(t["key"].tolist(), t["payload"].tolist())]
    return list(zip(t["key"].tolist(), t["payload"].tolist()))


def loop_merge(runs, width):
    """heapq.merge of the runs as tuples of Python integers."""
    out = list(heapq.merge(*[_pytuples(r) for r in runs]))
    return tup(width, [x[0] for x in out], [x[-1] for x in out])


def numpy_count(r, s):
    """sum_k |R_k| |S_k| as a Python integer."""
    kr, cr = np.unique(r["key"], return_counts=True)
    ks, cs = np.unique(s["key"], return_counts=True)
    both, ir, js = np.intersect1d(kr, ks, assume_unique=True, return_indices=True)
    return sum(int(a) * int(b) for a, b in zip(cr[ir].tolist(), cs[js].tolist()))


def loop_count(r, s):
    """The same from two dictionaries of Python integers."""
    cr, total = {}, 0
    for k in r["key"].tolist():
        cr[k] = cr.get(k, 0) + 1
    for k in s["key"].tolist():
        total += cr.get(k, 0)
    return total


# ---------------------------------------------------------------------------
# restatement of multiway_merge / multiway_merge_buckets
# ---------------------------------------------------------------------------
def key_u(keys):
    """The order-preserving unsigned form of int64 keys (key_u of smj_common.hpp)."""
    return np.asarray(keys, np.int64).view(np.uint64) ^ np.uint64(1 << 63)


def decide(width, runs):
    """What multiway_merge does with the runs: {"form": "none" | "buckets" |
    "tree", "k", "D", "L", "s", "sizes" (tuples per bucket), "queued" (the
    buckets above KM_CAP, ascending)}.  D, L and s are 0 and sizes and queued
    are empty for the forms without buckets."""
    k, total = len(runs), sum(len(r) for r in runs)
    d = {"form": "none", "k": k, "D": 0, "L": 0, "s": 0, "sizes": [], "queued": []}
    if total == 0:
        return d
    if not 3 <= k <= KM_KMAX:
        d["form"] = "tree"
        return d
    C = cap(width)
    D = 0
    while D < 24 and (total >> D) > C // 2:
        D += 1
    # the runs are sorted: the key range is that of their first and last tuples
    lo = min(int(key_u(r["key"][:1])[0]) for r in runs if len(r))
    hi = max(int(key_u(r["key"][-1:])[0]) for r in runs if len(r))
    L = (hi - lo).bit_length()
    s = max(L - D, 0)
    sizes = [0] * (1 << D)
    for r in runs:
        if len(r):
            rel = key_u(r["key"]) - np.uint64(lo)
            b = (rel >> np.uint64(s)) if s < 64 else np.zeros(len(r), np.uint64)
            cnt = np.bincount(b.astype(np.int64), minlength=1 << D)
            assert len(cnt) == 1 << D
            sizes = [x + int(y) for x, y in zip(sizes, cnt.tolist())]
    d.update(form="buckets", D=D, L=L, s=s, sizes=sizes,
             queued=[b for b, x in enumerate(sizes) if x > C])
    return d


def record_of(dec):
    """The smj_merge_stats a decision promises (Library.merge_stats)."""
    return {"form": dec["form"], "k": dec["k"], "D": dec["D"], "queued": len(dec["queued"])}


# ---------------------------------------------------------------------------
# 2-way cases: (content, n, split) -> (a, b)
# ---------------------------------------------------------------------------
SIZES2 = (MG_TILE - 1, MG_TILE, MG_TILE + 1, 2 * MG_TILE, 2 * MG_TILE + 1)
SPLITS = ("0_n", "n_0", "1_nm1", "nm1_1", "half")
CONTENTS = ("interleaved", "a_below_b", "b_below_a", "one_value", "one_key_a_above",
            "end_keys", "sign_straddle")


def contents(width):
    """sign_straddle is about the packed word of the 8-byte tuple."""
    return CONTENTS if width == 8 else CONTENTS[:-1]


def split(n, name):
    la = {"0_n": 0, "n_0": n, "1_nm1": 1, "nm1_1": n - 1, "half": n // 2}[name]
    return la, n - la


def two_way(width, content, n, sp):
    """The sorted inputs (a, b) of a 2-way case, la + lb = n."""
    la, lb = split(n, sp)
    seed = 7000 + 31 * n + 5 * SPLITS.index(sp) + 977 * CONTENTS.index(content)
    lo, hi = limits(width)
    a, b = rand_tuples(width, la, seed), rand_tuples(width, lb, seed + 1)
    rng = np.random.default_rng(seed)
    if content == "interleaved":
        a["key"], b["key"] = rng.integers(0, 3000, la), rng.integers(0, 3000, lb)
    elif content == "a_below_b":
        a["key"], b["key"] = rng.integers(-500, 0, la), rng.integers(0, 500, lb)
    elif content == "b_below_a":
        a["key"], b["key"] = rng.integers(0, 500, la), rng.integers(-500, 0, lb)
    elif content == "one_value":
        a, b = tup(width, [7] * la, -3), tup(width, [7] * lb, -3)
    elif content == "one_key_a_above":
        a = tup(width, [7] * la, lb + 10 + np.arange(la))
        b = tup(width, [7] * lb, np.arange(lb))
    elif content == "end_keys":
        a["key"], b["key"] = rng.choice([lo, hi], la), rng.choice([lo, hi], lb)
    elif content == "sign_straddle":
        a = tup(width, [7] * la, rng.integers(-1000, 1000, la))
        b = tup(width, [7] * lb, rng.integers(-1000, 1000, lb))
    else:
        raise KeyError(content)
    return srt(a), srt(b)


def check_two_way(width, content, a, b):
    """The content holds what its name promises (both inputs are sorted
    whatever the content: test_merge_cases.py checks that)."""
    lo, hi = limits(width)
    both = np.concatenate([a, b])
    if content == "interleaved" and len(a) > 1 and len(b) > 1:
        assert a["key"][0] < b["key"][-1] and b["key"][0] < a["key"][-1]
    if content == "a_below_b" and len(a) and len(b):
        assert a["key"][-1] < b["key"][0]
    if content == "b_below_a" and len(a) and len(b):
        assert b["key"][-1] < a["key"][0]
    if content == "one_value":
        assert len(np.unique(both)) == 1
    if content == "one_key_a_above":
        assert len(np.unique(both["key"])) == 1
        if len(a) and len(b):
            assert a["payload"].min() > b["payload"].max() >= 0
    if content == "end_keys":
        assert set(np.unique(both["key"]).tolist()) == {lo, hi}
    if content == "sign_straddle":
        assert len(np.unique(both["key"])) == 1
        assert both["payload"].min() < 0 < both["payload"].max()
        # the packed word's order: the non-negative payloads first
        s = srt(both)["payload"]
        neg = np.flatnonzero(s < 0)
        assert neg[0] > 0 and np.array_equal(neg, np.arange(neg[0], len(s)))


# ---------------------------------------------------------------------------
# k-way cases: name -> function of the width giving (runs, promise).  The
# promise: the fields of decide() the case is about ("queued" as a count) and
# "disorder": the tuples of the named key (or of every key, True) come in
# gather order (run after run) out of the sorted order.
# ---------------------------------------------------------------------------
def deal(t, k, seed, into=None):
    """The tuples of t dealt at random to the runs `into` (default all) of k,
    each run sorted."""
    rng = np.random.default_rng(seed)
    into = list(range(k)) if into is None else list(into)
    who = rng.choice(into, len(t))
    return [srt(t[who == i]) for i in range(k)]


def blocks_descending(width, key, lens):
    """One key over len(lens) runs: run i's payloads all above run i + 1's."""
    tops = np.cumsum(lens[::-1])[::-1]
    return [tup(width, [key] * n, top - n + np.arange(n)) for n, top in zip(lens, tops)]


def spread(total, k):
    """total as k positive lengths, the first ones longer."""
    return [total // k + (1 if i < total % k else 0) for i in range(k)]


def case_d0_ends(width):
    C = cap(width)
    lo, hi = limits(width)
    t = rand_tuples(width, C // 2, 11)
    # (rand_tuples stays inside +-2^62 at 16 bytes: the full range here)
    t["key"] = np.random.default_rng(12).integers(lo, hi, len(t), dtype=np.int64, endpoint=True)
    t["key"][:2] = [lo, hi]
    return deal(t, 3, 13), {"form": "buckets", "D": 0, "L": 8 * width // 2, "queued": 0}


def case_one_tuple(width):
    t = rand_tuples(width, 1, 14)
    return [t, t[:0], t[:0]], {"form": "buckets", "D": 0, "L": 0, "queued": 0}


def one_key(total_of, k, D, queued):
    def make(width):
        total = total_of(cap(width))
        runs = blocks_descending(width, -41, spread(total, k))
        return runs, {"form": "buckets", "D": D, "L": 0, "queued": queued, "disorder": -41,
                      "sizes": {total}}
    return make


def long_run(copies):
    """D = 0 and exact digits; one key `copies` times over five runs."""
    def make(width):
        rng = np.random.default_rng(copies)
        keys = rng.permutation(4000)[:800] - 2000
        keys = keys[keys != 123]
        t = rand_tuples(width, len(keys), 15)
        t["key"] = keys
        runs = deal(t, 5, 16)
        hot = blocks_descending(width, 123, spread(copies, 5))
        runs = [srt(np.concatenate([r, h])) for r, h in zip(runs, hot)]
        return runs, {"form": "buckets", "D": 0, "queued": 0, "disorder": 123,
                      "max_L": KM_LOGNB, "copies": (123, copies)}
    return make


def case_coarse_cluster(width):
    """Digits of 2^g keys: 100 distinct keys of one digit and 40 of another,
    dealt to five runs, so each digit's tuples are gathered out of order."""
    g = 8 if width == 8 else 40
    base = -(1 << (11 + g)) + 3
    rng = np.random.default_rng(17)
    step = 1 << (g - 8)
    in_a = base + (7 << g) + rng.permutation(256)[:100].astype(np.int64) * step + (step > 1)
    in_b = base + (2900 << g) + rng.permutation(256)[:40].astype(np.int64) * step
    others = base + (rng.permutation(4096)[:300].astype(np.int64) << g) + 1
    others = others[~np.isin((others - base) >> g, [7, 2900])]
    keys = np.concatenate([[base, base + (1 << (12 + g)) - 1], in_a, in_b, others])
    t = rand_tuples(width, len(keys), 18)
    t["key"] = keys
    return deal(t, 5, 19), {"form": "buckets", "D": 0, "L": 12 + g, "queued": 0,
                            "digits": (g, base, {7: 100, 2900: 40})}


def case_two_hot(width):
    C = cap(width)
    rng = np.random.default_rng(20)
    h1, h2 = (3 << 16) + 5, (12 << 16) + 77
    between = h1 + 1 + rng.permutation(h2 - h1 - 1)[:3 * C]
    outside = np.concatenate([[0, (1 << 20) - 1], rng.permutation(h1 - 1)[:40] + 1,
                              h2 + 1 + rng.permutation((1 << 20) - h2 - 2)[:40]])
    t = rand_tuples(width, len(between), 21)
    t["key"] = between
    runs = deal(t, 7, 22, into=(0, 1, 2, 4, 5, 6))
    o = rand_tuples(width, len(outside), 23)
    o["key"] = outside
    ends = deal(o, 7, 24, into=(0, 6))
    runs = [np.concatenate([r, e]) for r, e in zip(runs, ends)]
    for i, n in zip((1, 2, 4, 5), spread(C + 10, 4)):
        for h in (h1, h2):
            runs[i] = np.concatenate([runs[i], tup(width, [h] * n, rng.integers(0, 3, n))])
    return [srt(r) for r in runs], {
        "form": "buckets", "D": 4, "L": 20, "queued": 2, "queued_buckets": [3, 12],
        "hot": ((h1, h2), (1, 2, 4, 5), C + 10)}


def case_narrow_range(width):
    C = cap(width)
    t = rand_tuples(width, 40 * C, 25, 0, 16)
    t["key"] = np.arange(len(t)) % 16
    return deal(t, 5, 26), {"form": "buckets", "D": 7, "L": 4, "s": 0, "queued": 16,
                            "sizes": {0, 5 * C // 2}}


def case_slice_2p21(width):
    n = (1 << 21) + 5
    run0 = np.concatenate([tup(width, [99], [5]), tup(width, [100] * n, 2 * np.arange(n))])
    inside = 2 * (np.arange(10) * 200003 + 17) + 1
    run1 = np.concatenate([tup(width, [100] * 10, inside), tup(width, [101], [-5])])
    return [run0, run1, run0[:0]], {
        "form": "buckets", "D": 10 if width == 8 else 11, "L": 2, "s": 0, "queued": 1,
        "queued_buckets": [1], "sizes": {0, 1, n + 10}}


def case_bucket_edges(width):
    C = cap(width)
    rng = np.random.default_rng(27)
    edges = np.concatenate([[b * (1 << 16) - 1] * 30 + [b * (1 << 16)] * 30
                            for b in (1, 5, 8, 15)])
    t = rand_tuples(width, 6 * C, 28, 0, 1 << 20)
    t["key"][:len(edges)] = edges
    t["key"][len(edges):len(edges) + 2] = [0, (1 << 20) - 1]
    return deal(t, 6, 29), {"form": "buckets", "D": 4, "L": 20, "s": 16, "queued": 0,
                            "edges": edges}


def case_full_range(width):
    C = cap(width)
    lo, hi = limits(width)
    t = rand_tuples(width, 8 * C, 30)
    t["key"] = np.random.default_rng(31).integers(lo, hi, len(t), dtype=np.int64, endpoint=True)
    t["key"][:2] = [lo, hi]
    return deal(t, 8, 32), {"form": "buckets", "D": 4, "L": 8 * width // 2, "queued": 0}


def tree_one_run(n):
    def make(width):
        return [srt(rand_tuples(width, n, 33 + n, -50, 50))], {"form": "tree"}
    return make


def tree_two_runs(n):
    def make(width):
        return list(two_way(width, "interleaved", n, "half")), {"form": "tree"}
    return make


def case_tree_k257(width):
    e = np.zeros(0, DT[width])
    runs = [e] * 257
    runs[100], runs[256] = two_way(width, "interleaved", MG_TILE + 1, "half")
    return runs, {"form": "tree"}


def case_no_tuples(width):
    e = np.zeros(0, DT[width])
    return [e, e, e], {"form": "none"}


KWAY = {
    "d0_ends": case_d0_ends,
    "one_tuple": case_one_tuple,
    "one_key_half": one_key(lambda C: C // 2, 4, 0, 0),
    "one_key_half_p1": one_key(lambda C: C // 2 + 1, 4, 1, 0),
    "one_key_cap": one_key(lambda C: C, 4, 1, 0),
    "one_key_cap_p1": one_key(lambda C: C + 1, 4, 1, 1),
    "one_key_cap_k256": one_key(lambda C: C, 256, 1, 0),
    "one_key_cap_p1_k256": one_key(lambda C: C + 1, 256, 1, 1),
    "run64": long_run(KM_RUNMAX),
    "run65": long_run(KM_RUNMAX + 1),
    "coarse_cluster": case_coarse_cluster,
    "two_hot": case_two_hot,
    "narrow_range": case_narrow_range,
    "slice_2p21": case_slice_2p21,
    "bucket_edges": case_bucket_edges,
    "full_range": case_full_range,
    "tree_k1_n1": tree_one_run(1),
    "tree_k1_n2049": tree_one_run(MG_TILE + 1),
    "tree_k257": case_tree_k257,
    "no_tuples": case_no_tuples,
}
KWAY.update({f"tree_k2_n{n}": tree_two_runs(n) for n in SIZES2})
# checked against the oracle only (a Python loop over 2M tuples is slow)
LARGE = ("slice_2p21",)


def gather_order(runs):
    return np.concatenate(runs)


def check_promise(width, name, runs, promise):
    """The case holds what it promises, by decide() and by its tuples."""
    C = cap(width)
    dec = decide(width, runs)
    for f in ("form", "D", "L", "s"):
        if f in promise:
            assert dec[f] == promise[f], (name, f, dec[f], promise[f])
    if promise["form"] != "buckets":
        assert (dec["D"], dec["queued"], dec["sizes"]) == (0, [], [])
        return dec
    assert len(dec["queued"]) == promise["queued"], (name, dec["queued"])
    assert sum(dec["sizes"]) == sum(len(r) for r in runs)
    if promise["D"] == 0:
        assert sum(len(r) for r in runs) <= C // 2
    if "max_L" in promise:
        assert dec["L"] <= promise["max_L"]
    if "queued_buckets" in promise:
        assert dec["queued"] == promise["queued_buckets"]
    if "sizes" in promise:
        assert set(dec["sizes"]) - {0} == promise["sizes"] - {0}, (name, set(dec["sizes"]))
    allt = gather_order(runs)
    if "disorder" in promise:
        mine = allt[allt["key"] == promise["disorder"]]
        assert len(mine) > 1 and not np.array_equal(mine, srt(mine)), name
    if "copies" in promise:
        key, copies = promise["copies"]
        keys, cnt = np.unique(allt["key"], return_counts=True)
        assert cnt.max() == copies and keys[cnt.argmax()] == key and (cnt > 1).sum() == 1
    if "digits" in promise:   # coarse digits: (key - min) >> g, s3 = g > 0
        g, base, want = promise["digits"]
        assert dec["s"] - KM_LOGNB == g >= 8 and int(allt["key"].min()) == base
        dg = (allt["key"].astype(np.int64) - base) >> g
        for digit, n in want.items():
            mine = allt[dg == digit]
            assert len(mine) == n == len(np.unique(mine["key"]))
            assert not np.array_equal(mine, srt(mine))
        assert sorted(want.values())[-1] > KM_RUNMAX >= sorted(want.values())[0]
    if "hot" in promise:
        hot, where, n = promise["hot"]
        for h in hot:
            per_run = [int((r["key"] == h).sum()) for r in runs]
            assert sum(per_run) == n > C
            assert [i for i, x in enumerate(per_run) if x] == list(where)
            mine = allt[allt["key"] == h]
            assert set(mine["payload"].tolist()) == {0, 1, 2}
        assert len(runs) == 7 and len(runs[3]) == 0 and len(runs[0]) and len(runs[6])
        assert sum(len(r) for r in runs) - 2 * n >= 3 * C
    if "edges" in promise:
        keys, cnt = np.unique(allt["key"], return_counts=True)
        for e in np.unique(promise["edges"]).tolist():
            assert cnt[keys == e][0] >= 30
    if name == "slice_2p21":
        assert len(runs[0]) > 1 << 21 and len(runs[2]) == 0
        p0, p1 = runs[0]["payload"][1:], runs[1]["payload"][:10]
        assert p0[0] < p1.min() and p1.max() < p0[-1]
    if name.endswith("k256"):
        assert len(runs) == KM_KMAX and all(len(r) for r in runs)
    return dec


# ---------------------------------------------------------------------------
# merge-join count cases: name -> function of the width giving (r, s)
# ---------------------------------------------------------------------------
def count_one_key(width):
    n = 65537   # n^2 > 2^32
    return (srt(tup(width, [9] * n, np.arange(n))), srt(tup(width, [9] * n, -np.arange(n))))


def count_stride(width):
    """More S tuples than the largest grid has threads, keys distinct; R holds
    every third, the last ones past the grid's first trip."""
    ns = MJ_GRID + 300
    s = rand_tuples(width, ns, 34)
    s["key"] = np.arange(ns, dtype=np.int64) * 2 - ns
    r = rand_tuples(width, len(s[2::3]), 35)
    r["key"] = s["key"][2::3]
    return r, s


def count_end_keys(width):
    lo, hi = limits(width)
    r = rand_tuples(width, 8, 36)
    r["key"] = [lo] * 3 + [hi] * 5
    s = rand_tuples(width, 6, 37)
    s["key"] = [lo] * 4 + [hi] * 2
    return srt(r), srt(s)


def count_empty_r(width):
    return np.zeros(0, DT[width]), srt(rand_tuples(width, 100, 38, 0, 9))


def count_empty_s(width):
    return srt(rand_tuples(width, 100, 39, 0, 9)), np.zeros(0, DT[width])


COUNTS = {"one_key": count_one_key, "stride": count_stride, "end_keys": count_end_keys,
          "empty_r": count_empty_r, "empty_s": count_empty_s}
COUNT_PROMISE = {"one_key": 65537 ** 2, "stride": (MJ_GRID + 300 - 2 + 2) // 3,
                 "end_keys": 3 * 4 + 5 * 2, "empty_r": 0, "empty_s": 0}
COUNT_LARGE = ("stride",)
COUNTER_START = 5

_kway, _kexp, _two, _cnt = {}, {}, {}, {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def kway_inputs(width, name):
    """(runs, promise) of a k-way case, computed once and read-only."""
    if (width, name) not in _kway:
        runs, promise = KWAY[name](width)
        _kway[width, name] = (list(_frozen(*[np.ascontiguousarray(r) for r in runs])), promise)
    return _kway[width, name]


def kway_expected(width, name):
    if (width, name) not in _kexp:
        _kexp[width, name] = _frozen(numpy_merge(kway_inputs(width, name)[0], width))[0]
    return _kexp[width, name]


def two_way_inputs(width, content, n, sp):
    """(a, b, expected) of a 2-way case, computed once and read-only."""
    key = (width, content, n, sp)
    if key not in _two:
        a, b = two_way(width, content, n, sp)
        _two[key] = _frozen(a, b, numpy_merge([a, b], width))
    return _two[key]


def count_inputs(width, name):
    """(r, s, expected count) of a count case, computed once and read-only."""
    if (width, name) not in _cnt:
        r, s = COUNTS[name](width)
        _cnt[width, name] = _frozen(r, s) + (numpy_count(r, s),)
    return _cnt[width, name]
