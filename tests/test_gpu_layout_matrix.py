"""Layout x plan x shape matrix of the device sort and join.

smj_dev_join and smj_dev_sort both run through device_bucket (capi.hip), which
picks one of six intermediate layouts (32-bit words, 48-bit planes, 64-bit
words, 12-byte elements, sampled tuples, exact tuples), one of the ways to get
the plan (key-range hint, verified size guess, exact min/max pass, device
sample) and the level widths D1/D2/D3 from n and fanout_bits.  Every
combination is another kernel or another instance of k_tilepass / k_groupsort.
The cases below walk that space at the sizes where a shift, a mask, a tile
edge or a table size can go wrong.

Expected values are plain numpy (sorted relations and the match count),
cross-checked once with the oracle where the count is small enough for its
one-match-per-step merge join.  Every case also checks: the 64 sentinel
tuples in front of and behind both outputs, that the count is overwritten and not added to,
that the inputs are untouched, a second call on the same workspace, the
layout the call finished in and (kernel trace) whether the exact partition
and the skew kernels ran.

The expected layouts are written by hand in the tables, read from
device_bucket (layout_caps, p48_fits) and the ladder it walks
(csrc/layout_policy.hpp: first_rung, after_void, layout_of); the CPU walk of
these tables through that header is tests/test_layout_policy.py.
"x!" means: layout x after the exact partition (rung Exact: k_hist ran).

What the tables had to learn from the code (corrections to the first
reading; none of them changes a result, only the layout a call ends in):

* A sampled attempt gives every partition eight shard regions of
  est/8 * 9/8 + 1024 elements (k_regions), and scatter workgroup i fills shard
  i % 8 (k_scatter_res).  With fewer than eight workgroups, or a workgroup
  count that is no multiple of eight, the shards are filled unevenly; a shard
  that receives more than its region raises the overflow flag, the attempt's
  result is discarded and the call goes on to the sampled tuples (rung Sampled),
  which overflow likewise, and ends in the exact partition (Exact, "tuples!").
  One workgroup (n up to one scatter tile) overflows as soon as a partition
  holds more than about 1190 tuples: 2000 and 2048 tuples at D1 = 0, the sorts
  of 4096 tuples.  A handful of workgroups overflow when partitions are large
  (fan-out 1 and 4 at 40 000 to 300 000 tuples, the 71 000-tuple skew case).
  The results are right either way, so these cases expect "tuples!"; the
  shapes named *_fit are additions of this file at which the same layouts
  complete (1100 tuples: one workgroup within the slack; 393 216 tuples:
  eight times every layout's scatter tile, all shards level).
* Empty and one-key inputs have s1 = 0: no packed word is usable, 16-byte
  tuples take the 12-byte elements (span 0 < 2^32), 8-byte tuples the sampled
  tuples.
* p48_fits is computed once per call, from the first plan.  A sort whose
  guessed plan 1..n is replaced by the exact range keeps the guess's answer,
  and a shape that has failed the 32-bit words skips them on later calls, so
  the first and the second call of one shape can end in different layouts
  ("a,b" in a table: a on a fresh workspace, b afterwards).  See group B,
  full8 and s1_32_fit.
"""
import collections
import zlib

import numpy as np
import pytest

# SMJ_LAYOUT_* of include/smj.h (test_flag_values pins them to the binding's)
NO_P48, NO_PACKED, NO_SAMPLED, SAMPLE_PLAN, NO_P32, NO_P96 = 1, 2, 4, 8, 16, 32
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
CANARY = 64          # sentinel tuples behind every output
SENTINEL = 0x5A5A5A5A
DTYPES = {8: np.dtype([("payload", "<i4"), ("key", "<i4")]),
          16: np.dtype([("payload", "<i8"), ("key", "<i8")])}

# ---------------------------------------------------------------------------
# the plan, restated
# ---------------------------------------------------------------------------
K_GROUP_TARGET = 2048      # bucketsort.hip kGroupTarget (GS_CAP 2560 * 4 / 5)
K_TILE_TUPLES = 16384      # bucketsort.hip SMJ_PLAN_TILE
K_NARROW_DIGIT_BITS = 12   # smj_internal.hpp
K_MAX_D2 = 10              # smj_internal.hpp
K_GROUP_D3MAX = 11         # bucketsort.hip GS_D3MAX

Plan = collections.namedtuple("Plan", "base span L B D1 D2 D3 s1 s2 s3")


def ceil_log2(x):
    b = 0
    while b < 63 and (1 << b) < x:
        b += 1
    return b


def choose_levels(n, want_d1, tile=K_TILE_TUPLES):
    """choose_levels of capi.hip: (B, D1, D2, D2cap) for a
    larger relation of n tuples and fanout_bits want_d1 (0: the default 8)."""
    t = K_GROUP_TARGET
    B = ceil_log2((n + t - 1) // t) if n > t else 0
    d1 = want_d1 if want_d1 else 8
    while d1 < K_NARROW_DIGIT_BITS and (n >> d1) > 192 * tile:
        d1 += 1
    d1 = min(d1, B, K_NARROW_DIGIT_BITS)
    d2 = min(B - d1 if B > d1 else 0, K_MAX_D2)
    d2cap = d2 + 2 if d2 + 2 < K_MAX_D2 else (d2 if d2 > K_MAX_D2 else K_MAX_D2)
    return B, d1, d2, d2cap


def make_plan(kmin, kmax, levels, d3max=K_GROUP_D3MAX):
    """make_plan of smj_common.hpp on choose_levels' result.
    Python integers: key_u(kmax) - key_u(kmin) is kmax - kmin."""
    B, D1, D2, D2cap = levels
    width = kmax - kmin if kmax >= kmin else 0
    L = width.bit_length()
    assert L <= 64
    s1 = L - D1 if L > D1 else 0
    d2 = min(D2, s1)
    s2 = s1 - d2
    if s2 > d3max and d2 < D2cap:
        extra = min(s2 - d3max, D2cap - d2)
        d2 += extra
        s2 -= extra
    D3 = min(s2, d3max)
    return Plan(kmin, (1 << L) - 1, L, B, D1, d2, D3, s1, s2, s2 - D3)


def layout_usable(layout, width, plan, flags, hinted):
    """usable() of the layout (smj_common.hpp) and the conditions device_bucket
    adds (capi.hip layout_caps); tuples always apply."""
    nb = 1 << plan.D1
    words_ok = hinted and not (flags & (NO_SAMPLED | NO_PACKED)) and plan.D1 <= 10
    if layout == "p32":
        return words_ok and not (flags & NO_P32) and 1 <= plan.s1 <= 31
    if layout == "p48":
        return words_ok and not (flags & NO_P48) and 1 <= plan.s1 <= 32 and nb <= 512
    if layout == "words":
        return width == 16 and words_ok and 1 <= plan.s1 <= 32
    if layout == "p96":
        return (width == 16 and hinted and not (flags & (NO_SAMPLED | NO_P96)) and
                plan.D1 <= 10 and plan.span < (1 << 32))
    return layout in ("tuples", "none")


WORD_BITS = {"p32": 32, "p48": 48, "words": 64}


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
class Case:
    """One call: `kind` join (R and S) or sort (R alone).  keys(rng) gives the
    key arrays, pay names the payloads (see payloads()), hint the key range
    passed to the join (None: none), expect[width] = "layout" or "layout!"
    (None: the case does not exist at that width, `why`)."""

    def __init__(self, name, kind, nR, nS, fanout, flags, hint, keys, pay, expect,
                 skew=False, why=""):
        self.name, self.kind, self.nR, self.nS = name, kind, nR, nS
        self.fanout, self.flags, self.hint, self.keys, self.pay = fanout, flags, hint, keys, pay
        self.expect, self.skew, self.why = expect, skew, why

    @property
    def ns(self):
        return (self.nR, self.nS) if self.kind == "join" else (self.nR,)

    def plan_range(self, width):
        """The key range device_bucket plans from, as far as the case table
        knows it: the hint, else the sort's size guess, else the data's range
        (key_range; a device-sampled plan covers at least that)."""
        if self.hint is not None:
            return self.hint
        if self.kind == "sort" and not self.keys_break_guess:
            return (1, max(self.nR, 1))
        return self.key_span[width]

    keys_break_guess = False
    key_span = None

    def plan(self, width):
        lo, hi = self.plan_range(width)
        return make_plan(lo, hi, choose_levels(max(self.ns), self.fanout))

    def _expect(self, width, call):
        # "a,b": a on a fresh workspace, b on the calls after it
        e = self.expect[width].split(",")
        return e[min(call, len(e) - 1)]

    def layout(self, width, call=0):
        return self._expect(width, call).rstrip("!")

    def exact(self, width, call=0):
        return self._expect(width, call).endswith("!")

    def pay_bits(self, width):
        """Bits of the widest payload (as the unsigned value the words hold),
        None for full-width ones."""
        s1 = self.plan(width).s1
        full = 31 if width == 8 else 63
        if self.pay in WORD_BITS:
            return max(min(WORD_BITS[self.pay] - s1, full), 1)
        if self.pay == "rowid":
            return max(max(self.ns) - 1, 1).bit_length()
        if self.pay == "bit":
            return 1
        assert self.pay == "full"
        return None


def _seed(*parts):
    return np.random.default_rng([zlib.crc32(p.encode()) if isinstance(p, str) else p
                                  for p in parts])


def payloads(case, width, n, rng):
    """"p32" / "p48" / "words": random values of exactly the bits that layout
    holds under the case's plan (X - s1; at most the non-negative range), the
    largest one present.  "full": random full-width values, both ends present.
    "rowid": the row number.  "bit": 0 or 1."""
    dt = DTYPES[width]["payload"]
    if case.pay == "rowid":
        return np.arange(n, dtype=dt)
    if case.pay == "full":
        info = np.iinfo(dt)
        p = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        p[:2] = (info.min, info.max)[:len(p[:2])]
        return p
    bits = case.pay_bits(width)
    p = rng.integers(0, 1 << bits, n, dtype=np.int64)
    if n:
        p[n // 2] = (1 << bits) - 1
    return p.astype(dt)


def relation(width, keys, pay):
    t = np.zeros(len(keys), DTYPES[width])
    t["key"] = keys
    t["payload"] = pay
    return t


def input_key(case, width):
    """What the input relations of a case depend on."""
    return (width, case.kind, case.nR, case.nS, case.keys.tag, case.pay, case.pay_bits(width),
            getattr(case, "fix", None))


def build(case, width):
    """The input relations of a case: [R, S] or [R]."""
    ks = case.keys(_seed(case.keys.tag, *case.ns), width, *case.ns)
    rng = _seed(case.pay, case.pay_bits(width) or 0, width, *case.ns)
    rels = [relation(width, k, payloads(case, width, len(k), rng)) for k in ks]
    if getattr(case, "fix", None) == "ident":
        # (test_gpu_skew_matrix) the tuples of a key all alike: its first payload
        for t in rels:
            _, first, inv = np.unique(t["key"], return_index=True, return_inverse=True)
            t["payload"] = t["payload"][first][inv]
    return rels


# ---- key generators: f(rng, width, nR[, nS]) -> key arrays ------------------
def dense_keys(rng, width, nR, nS=None):
    """R a permutation of 1..nR, S uniform draws from 1..max(nR, 1)."""
    kR = rng.permutation(nR).astype(np.int64) + 1
    if nS is None:
        return [kR]
    return [kR, rng.integers(1, max(nR, 1) + 1, nS, dtype=np.int64)]


dense_keys.tag = "dense"


def range_keys(lo, hi):
    """Uniform draws from [lo, hi] with both ends present in every relation;
    half of S repeats keys of R so that the join has matches."""
    def f(rng, width, nR, nS=None):
        kR = rng.integers(lo, hi, nR, dtype=np.int64, endpoint=True)
        kR[0], kR[-1] = lo, hi
        if nS is None:
            return [kR]
        kS = rng.integers(lo, hi, nS, dtype=np.int64, endpoint=True)
        kS[: nS // 2] = kR[rng.integers(0, nR, nS // 2)]
        kS[0], kS[-1] = hi, lo
        return [kR, kS]
    f.tag = f"range{lo}:{hi}"
    return f


def hot_keys(copies):
    """`copies` tuples of key 5 and the keys 1..1000 once each, shuffled."""
    def f(rng, width, nR, nS=None):
        out = []
        for _ in range(1 if nS is None else 2):
            k = np.concatenate([np.full(copies, 5, np.int64), np.arange(1, 1001, dtype=np.int64)])
            out.append(rng.permutation(k))
        return out
    f.tag = f"hot{copies}"
    return f


# ---- group A: forced layout x shape (hinted, dense keys) -------------------
# (nR, nS, fanout_bits): boundaries of kGroupTarget, the tiles, a level width
A_SHAPES = [
    ("empty", 0, 0, 8), ("r_empty", 0, 7, 8), ("s_empty", 7, 0, 8), ("one", 1, 1, 8),
    ("fit", 1100, 900, 8),             # added: D1 = 0, one workgroup within the slack
    ("group", 2048, 2048, 8),          # D1 = 0, one full group
    ("d1_1", 2049, 1, 8),              # D1 = 1
    ("tile", 16383, 16385, 8),         # D1 = 4, buckets around one tile
    ("d2_2", 40_000, 70_001, 4),       # D1 = 4, D2 = 2
    ("d2_7", 300_007, 150_001, 1),     # D1 = 1, D2 = 7
    ("d2_9", 1_050_000, 1_050_000, 1),  # D2 = 9: the 16-byte p48 case takes LayP40
    ("d2_10", 2_200_000, 2_200_000, 1),  # D2 = kMaxD2
]
A_GROUPS = {"small": ["empty", "r_empty", "s_empty", "one", "fit", "group", "d1_1", "tile"],
            "mid": ["d2_2", "d2_7"], "d2_9": ["d2_9"], "d2_10": ["d2_10"]}

# row: (flags, payloads, hinted, expected layout at 8 / 16 bytes where the
# row's layout applies), then per shape what the code does instead.
# s1 of the shapes: empty 0, r_empty / s_empty 3, one 0, fit 11, group 11,
# d1_1 11, tile 11, d2_2 13, d2_7 18, d2_9 20, d2_10 21.
A_ROWS = {
    "p32": (0, "p32", True, "p32", "p32"),
    "p48": (NO_P32, "p48", True, "p48", "p48"),
    "words": (NO_P32 | NO_P48, "words", True, None, "words"),
    "p96": (0, "full", True, None, "p96"),
    "tuples_sampled": (NO_PACKED | NO_P96, "full", True, "tuples", "tuples"),
    "tuples_exact": (NO_SAMPLED, "full", True, "tuples!", "tuples!"),
    "device_plan": (SAMPLE_PLAN, "full", False, "tuples", "tuples"),
    "device_plan_exact": (SAMPLE_PLAN | NO_SAMPLED, "full", False, "tuples!", "tuples!"),
}
# s1 = 0 (empty, one): no packed word (usable() needs s1 >= 1); 16 bytes then
# take p96 (rung Sampled, span 0), 8 bytes the sampled tuples
_S1_ZERO = {(8, "empty"): "tuples", (8, "one"): "tuples", (16, "empty"): "p96", (16, "one"): "p96"}
# A shard region overflows (module docstring) in every sampled attempt:
#   group  one scatter workgroup, one partition of 2048 tuples
#   d1_1   one workgroup; partition 0 holds the keys 1..2048 (s1 = 11)
# and with the 8-byte tuples' larger scatter tiles (12288 and 16384) also:
#   tile   S's first workgroup holds 16384 tuples, 2048 a partition
#   d2_2   6 or 5 workgroups, S's 16 partitions of ~4400 tuples
#   d2_7   2 partitions; R: 25 or 19 workgroups, S: 13 or 10
_OVF = {(w, s): "tuples!" for w in (8, 16) for s in ("group", "d1_1")}
_OVF.update({(8, s): "tuples!" for s in ("tile", "d2_2", "d2_7")})
# d2_7 at 16 bytes: the words (8192-element scatter tiles: S in 19 workgroups,
# three of them on shards 0 to 2) overflow, the attempt after them does not:
# 12-byte elements in 6144-element tiles (25 workgroups)
_OVF_WORDS = {**_OVF, (16, "d2_7"): "p96"}
A_INSTEAD = {
    "p32": {**_S1_ZERO, **_OVF_WORDS},
    "p48": {**_S1_ZERO, **_OVF_WORDS},
    "words": {(16, "empty"): "p96", (16, "one"): "p96", **_OVF_WORDS},
    "p96": {**_OVF},
    "tuples_sampled": {**_OVF},
    "tuples_exact": {},
    # the sampled plan's range is a little wider than the hint's (k_plan adds
    # 1/64 on both sides), its partitions differ: d2_2 stays within the shards
    "device_plan": {k: v for k, v in _OVF.items() if k != (8, "d2_2")},
    "device_plan_exact": {},
}


def group_a(row, shapes):
    flags, pay, hinted, e8, e16 = A_ROWS[row]
    out = []
    for name, nR, nS, fan in A_SHAPES:
        if name not in shapes:
            continue
        expect = {8: e8, 16: e16}
        for w in (8, 16):
            if expect[w] is not None:
                expect[w] = A_INSTEAD[row].get((w, name), expect[w])
        c = Case(f"A-{row}-{name}", "join", nR, nS, fan, flags,
                 (1, max(nR, nS, 1)) if hinted else None, dense_keys, pay, expect,
                 why="no such layout for 8-byte tuples")
        c.key_span = {8: (1, max(nR, 1)), 16: (1, max(nR, 1))}
        out.append(c)
    return out


# fan-out past the sampled scatter (D1 > 10): exact partition whatever the flags
A_FANOUT = [
    Case("A-fanout11", "join", 2_200_000, 500_000, 11, 0, (1, 2_200_000), dense_keys, "rowid",
         {8: "tuples!", 16: "tuples!"}),
    Case("A-fanout12", "join", 4_300_000, 4_300_000, 12, 0, (1, 4_300_000), dense_keys, "full",
         {8: "tuples!", 16: "tuples!"}),
]


# ---- group B: plan edges ----------------------------------------------------
def group_b():
    """Every key set at 2000 tuples (D1 = 0) and at 600 000 (D1 = 8, D2 = 1),
    through the join with its hint and through the sort of R.  The sort knows
    no hint: it guesses keys 1..n, which these keys break (kBadRange), and
    restarts with the exact range.  Expectations: per width, the layout of
    the join and of the sort (a missing entry: not run)."""
    def hint(l1, d1, lo=None):
        # a range of bit length s1 + D1 around 0 (or from lo)
        w = (1 << (l1 + d1)) - 1
        lo = -(w // 2) - 1 if lo is None else lo
        return (lo, lo + w)

    N0, N8 = 2000, 600_000
    rows = []

    def add(name, n, fan, h, keys_range, pay, exp, skew=(), why=""):
        lo, hi = keys_range
        for kind in ("join", "sort"):
            e = {w: (exp[w].get(kind) if exp.get(w) else None) for w in (8, 16)}
            if all(v is None for v in e.values()):
                continue
            c = Case(f"B-{name}-{n}-{kind}", kind, n, n, fan if kind == "join" else 0, 0,
                     h if kind == "join" else None, range_keys(lo, hi), pay, e,
                     skew=kind in skew, why=why)
            c.key_span = {8: (lo, hi), 16: (lo, hi)}
            c.keys_break_guess = not (1 <= lo and hi <= n)
            rows.append(c)

    T = "tuples!"
    # s1 = 0: one key, count n^2.  2000: the one partition overflows its shard.
    add("s1_0", N0, 8, (42, 42), (42, 42), "rowid",
        {8: {"join": T, "sort": T}, 16: {"join": T, "sort": T}})
    # 600 000 equal keys: one group far beyond LDS (skew path).  The sort's
    # guess 1..n holds key 42: s1 = 12, row ids fit the 32-bit words.
    add("s1_0", N8, 8, (42, 42), (42, 42), "rowid",
        {8: {"join": "tuples", "sort": "p32"}, 16: {"join": "p96", "sort": "p32"}},
        skew=("join", "sort"))
    # s1 = 1: two keys a partition
    add("s1_1", N0, 8, (-3, -2), (-3, -2), "rowid",
        {8: {"join": T, "sort": T}, 16: {"join": T, "sort": T}})
    add("s1_1", N8, 8, (-3, 508), (-3, 508), "rowid",
        {8: {"join": "p32", "sort": "p32"}, 16: {"join": "p32", "sort": "p32"}})
    # s1 = 31: one payload bit left in a 32-bit word
    add("s1_31", N0, 8, hint(31, 0), hint(31, 0), "bit",
        {8: {"join": T, "sort": T}, 16: {"join": T, "sort": T}})
    add("s1_31", N8, 8, hint(31, 8), hint(31, 8), "bit",
        {8: None, 16: {"join": "p32", "sort": "p32"}}, why="8-byte keys span at most 2^32")
    # s1 = 32: no 32-bit words, p48_fits false: 64-bit words (16 B), tuples (8 B)
    add("s1_32", N0, 8, hint(32, 0), hint(32, 0), "rowid",
        {8: {"join": T, "sort": T}, 16: {"join": T, "sort": T}})
    add("s1_32", N8, 8, hint(32, 8), hint(32, 8), "rowid",
        {8: None, 16: {"join": "words", "sort": "words"}}, why="8-byte keys span at most 2^32")
    # s1 = 33: no packed word, span >= 2^32: tuples
    add("s1_33", N0, 8, hint(33, 0), hint(33, 0), "rowid",
        {8: None, 16: {"join": T, "sort": T}}, why="8-byte keys span at most 2^32")
    add("s1_33", N8, 8, hint(33, 8), hint(33, 8), "rowid",
        {8: None, 16: {"join": "tuples", "sort": "tuples"}}, why="8-byte keys span at most 2^32")
    # L = 64 (16 B): s1 = 64 at D1 = 0, 56 at D1 = 8; with the hint and without
    for n, e in ((N0, T), (N8, "tuples")):
        add("l64", n, 8, (I64_MIN, I64_MAX), (I64_MIN, I64_MAX), "rowid",
            {8: None, 16: {"join": e, "sort": e}}, why="16-byte keys only")
        add("l64_nohint", n, 8, None, (I64_MIN, I64_MAX), "rowid",
            {8: None, 16: {"join": e}}, why="16-byte keys only")
    # the full 32-bit range (8 B): s1 = 32 at D1 = 0 (tuples), 24 at D1 = 8.
    # There the row ids need 20 bits: not the 8 of a 32-bit word, so the first
    # call goes on to the 48-bit planes and notes p32_fail for the shape.  The
    # second call skips the 32-bit words in plan_rung, and plan_rung takes
    # the 48-bit planes only where p48_fits (span < 2^(48 - s1), false here):
    # it runs on the sampled tuples.  Both are right; the layout differs.
    # The sort stays on the 48-bit planes: p48_fits is evaluated once, on the
    # guessed plan 1..n (span 2^20), and kept when the sort restarts with the
    # exact range (first reading: re-evaluated, hence tuples; the GPU said p48).
    for n, e in ((N0, T), (N8, "p48,tuples")):
        add("full8", n, 8, (I32_MIN, I32_MAX), (I32_MIN, I32_MAX), "rowid",
            {8: {"join": e, "sort": e.split(",")[0]}, 16: None}, why="the 8-byte key range")
        add("full8_nohint", n, 8, None, (I32_MIN, I32_MAX), "rowid",
            {8: {"join": e}, 16: None}, why="the 8-byte key range")
    # a hint narrower than the data: the words flag kBadRange, the tuples
    # clamp the keys to the end digits
    add("narrow", N0, 8, (1000, 2999), (1, 4000), "rowid",
        {8: {"join": T}, 16: {"join": T}})
    # additions: the D1 = 0 plans at a size whose one workgroup stays within
    # its shard (1100 tuples), so that the layouts themselves complete
    N1 = 1100
    add("s1_0_fit", N1, 8, (42, 42), (42, 42), "rowid",
        {8: {"join": "tuples", "sort": "p32"}, 16: {"join": "p96", "sort": "p32"}})
    add("s1_1_fit", N1, 8, (-3, -2), (-3, -2), "rowid",
        {8: {"join": "p32", "sort": "p32"}, 16: {"join": "p32", "sort": "p32"}})
    add("s1_31_fit", N1, 8, hint(31, 0), hint(31, 0), "bit",
        {8: {"join": "p32", "sort": "p32"}, 16: {"join": "p32", "sort": "p32"}})
    # (the sort: p48_fits from the guessed plan 1..n holds after the restart,
    # as in full8; 48 - 32 = 16 bits hold the row ids.  At 600 000 they do not
    # and the 48-bit attempt hands over to the 64-bit words.)
    add("s1_32_fit", N1, 8, hint(32, 0), hint(32, 0), "rowid",
        {8: {"join": "tuples", "sort": "p48"}, 16: {"join": "words", "sort": "p48"}})
    add("s1_33_fit", N1, 8, hint(33, 0), hint(33, 0), "rowid",
        {8: None, 16: {"join": "tuples", "sort": "tuples"}}, why="8-byte keys span at most 2^32")
    add("l64_fit", N1, 8, (I64_MIN, I64_MAX), (I64_MIN, I64_MAX), "rowid",
        {8: None, 16: {"join": "tuples", "sort": "tuples"}}, why="16-byte keys only")
    add("narrow_fit", N1, 8, (1000, 2999), (1, 4000), "rowid",
        {8: {"join": "tuples"}, 16: {"join": "tuples!"}})
    return rows


# ---- group C: dev_sort under every layout -----------------------------------
C_SIZES = [0, 1, 2, 15, 16, 255, 4096, 16384, 49229]  # 49229 = 3 * 16384 + 77
C_ROWS = {"p32": (0, "p32"), "p48": (NO_P32, "p48"), "words": (NO_P32 | NO_P48, "words"),
          "p96": (0, "full"), "tuples": (NO_PACKED | NO_P96, "full")}


def group_c(row):
    flags, pay = C_ROWS[row]
    out = []
    for n in C_SIZES:
        lay8 = {"p32": "p32", "p48": "p48", "words": None, "p96": None, "tuples": "tuples"}[row]
        lay16 = row
        if n == 0:       # smj_dev_sort returns before device_bucket
            lay8 = lay8 and "none"
            lay16 = "none"
        elif n == 1:     # s1 = 0: no packed word
            lay8 = lay8 and "tuples"
            lay16 = "tuples" if row == "tuples" else "p96"
        elif n == 4096:  # one workgroup, 2048 tuples a partition: shard overflow
            lay8 = lay8 and "tuples!"
            lay16 = "tuples!"
        elif n == 16384:  # 8 bytes: still one workgroup (tiles of 12288 / 16384)
            lay8 = lay8 and "tuples!"
        c = Case(f"C-{row}-{n}", "sort", n, n, 0, flags, None, dense_keys, pay,
                 {8: lay8, 16: lay16}, why="no such layout for 8-byte tuples")
        out.append(c)
    return out


# ---- group D: fused count above 2^32 ----------------------------------------
D_ROWS = {"p48": (NO_P32, "p48"), "words": (NO_P32 | NO_P48, "words"), "p96": (0, "full"),
          "tuples": (NO_PACKED | NO_P96, "full")}
D_FIT = 8 * 49152 - 1000  # copies: n = 8 x the lcm of the layouts' scatter tiles


def group_d(row):
    flags, pay = D_ROWS[row]
    lay8 = {"p48": "p48", "words": None, "p96": None, "tuples": "tuples"}[row]
    out = []
    for name, copies, ovf in (("hot", 70_000, True), ("hot_fit", D_FIT, False)):
        n = copies + 1000
        e = {8: lay8 and ("tuples!" if ovf else lay8), 16: "tuples!" if ovf else row}
        c = Case(f"D-{row}-{name}", "join", n, n, 8, flags, (1, 1000), hot_keys(copies), pay, e,
                 skew=True, why="no such layout for 8-byte tuples")
        c.key_span = {8: (1, 1000), 16: (1, 1000)}
        out.append(c)
    return out


def all_cases():
    out = []
    for row in A_ROWS:
        out += group_a(row, [s[0] for s in A_SHAPES])
    out += A_FANOUT + group_b()
    for row in C_ROWS:
        out += group_c(row)
    for row in D_ROWS:
        out += group_d(row)
    return out


# ---------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------
def test_flag_values():
    import smj
    assert (smj.LAYOUT_NO_P48, smj.LAYOUT_NO_PACKED, smj.LAYOUT_NO_SAMPLED,
            smj.LAYOUT_SAMPLE_PLAN, smj.LAYOUT_NO_P32, smj.LAYOUT_NO_P96) == \
        (NO_P48, NO_PACKED, NO_SAMPLED, SAMPLE_PLAN, NO_P32, NO_P96)
    assert smj.LAYOUTS_USED == ("tuples", "words", "p48", "p32", "p96")


def test_plan_restatement():
    """Spot values of choose_levels and make_plan against the source's own
    comments and tests (test_gpu_tilepass48: 1.1M tuples in 4 buckets leave 8
    level-2 bits; a 2^21 key range at D1 = 2 has s1 = 19)."""
    assert choose_levels(2048, 8) == (0, 0, 0, 2)
    assert choose_levels(2049, 8) == (1, 1, 0, 2)
    assert choose_levels(1_100_000, 2) == (10, 2, 8, 10)
    assert choose_levels(1 << 27, 0)[1:3] == (8, 8)
    assert choose_levels(1 << 30, 0)[1] == 9          # 192 tiles a bucket: 2^9 partitions
    p = make_plan(1, 1 << 21, (10, 2, 8, 10))
    assert (p.L, p.s1, p.D2, p.s2, p.D3, p.s3) == (21, 19, 8, 11, 11, 0)
    p = make_plan(I64_MIN, I64_MAX, (0, 0, 0, 2))
    assert (p.L, p.span, p.s1, p.D2, p.s2, p.D3, p.s3) == (64, (1 << 64) - 1, 64, 2, 62, 11, 51)
    p = make_plan(42, 42, (9, 8, 1, 3))
    assert (p.L, p.span, p.s1, p.D2, p.D3, p.s3) == (0, 0, 0, 0, 0, 0)


def test_case_table_reaches_edges():
    """The plan values of every case: the tables as a whole must reach the
    level widths and shifts named in the issue, and every hand-written layout
    must be one its own usable() and payload conditions allow under the
    restated plan."""
    d1, d2, s1, s3, L = set(), set(), set(), set(), set()
    names = set()
    for c in all_cases():
        assert c.name not in names, c.name
        names.add(c.name)
        for w, call in ((8, 0), (8, 1), (16, 0), (16, 1)):
            if c.expect[w] is None:
                assert c.why, c.name
                continue
            lay = c.layout(w, call)
            if lay == "none":
                assert c.kind == "sort" and c.nR == 0, c.name
                continue
            p = c.plan(w)
            d1.add(p.D1)
            d2.add(p.D2)
            s1.add((p.s1, p.D1, w))
            s3.add(p.s3 > 0)
            L.add(p.L)
            hinted = c.hint is not None or not (c.flags & SAMPLE_PLAN)
            assert layout_usable(lay, w, p, c.flags, hinted), (c.name, w, lay, p)
            if lay in WORD_BITS:
                bits = c.pay_bits(w)
                assert bits is not None and bits <= WORD_BITS[lay] - p.s1, (c.name, w, lay, p)
            if c.exact(w, call):
                assert lay == "tuples", c.name
            if p.D1 > 10 or (c.flags & NO_SAMPLED):
                assert c.exact(w, call), c.name
            if w == 8:
                assert p.L <= 32, c.name
    assert {0, 1, 4, 8, 11} <= d1, d1
    assert {0, 2, 7, 9, 10} <= d2, d2
    assert {0, 1, 31, 32, 33} <= {s for s, _, _ in s1}, s1
    assert (64, 0, 16) in s1
    assert not any(s == 64 and (d, w) != (0, 16) for s, d, w in s1)
    assert s3 == {False, True}
    assert 64 in L


# ---------------------------------------------------------------------------
# expected values: plain numpy
# ---------------------------------------------------------------------------
def np_sorted(width, t):
    """16 bytes: ascending (key, payload), both signed.  8 bytes: ascending
    signed key, then the payload as unsigned 32-bit (the packed-word order of
    smj.h)."""
    if width == 8:
        # one signed 64-bit word a tuple: the key above the unsigned payload
        w = np.sort((t["key"].astype(np.int64) << 32) | t["payload"].view(np.uint32))
        return relation(8, (w >> 32).astype(np.int32), (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    if len(t) < 1 << 20:
        return t[np.lexsort((t["payload"], t["key"]))]
    # the same order from three plain sorts (lexsort's stable passes take
    # seconds at millions of tuples): rank of the key * n + rank of the
    # payload.  Payload ties get arbitrary ranks; under equal keys they are
    # identical tuples, whose order does not show.
    n = len(t)
    pay_rank = np.empty(n, np.int64)
    pay_rank[np.argsort(t["payload"])] = np.arange(n, dtype=np.int64)
    kmin, kmax = int(t["key"].min()), int(t["key"].max())
    if (kmax - kmin + 1) * n < 1 << 62:
        key_rank = t["key"] - kmin   # monotone in the key, and the product fits
    else:
        _, key_rank = np.unique(t["key"], return_inverse=True)
    return t[np.argsort(key_rank.astype(np.int64) * n + pay_rank)]


def np_count(R, S):
    """Sum over the keys of cR(k) * cS(k).  Counts below 2^15 on both sides
    multiply and add in int64 without wrapping (fewer than 2^32 keys, each
    product below 2^30); every other key is added in Python integers."""
    kr, cr = np.unique(R["key"], return_counts=True)
    ks, cs = np.unique(S["key"], return_counts=True)
    _, ir, i_s = np.intersect1d(kr, ks, assume_unique=True, return_indices=True)
    a, b = cr[ir].astype(np.int64), cs[i_s].astype(np.int64)
    small = (a < 1 << 15) & (b < 1 << 15)
    total = int((a[small] * b[small]).sum())
    for x, y in zip(a[~small].tolist(), b[~small].tolist()):
        total += x * y
    return total


_EXPECTED = collections.OrderedDict()


def expected(case, width, orc):
    """(inputs, sorted relations, count) of a case, computed once per (width,
    input) and pinned to the oracle where its merge join can count that far.
    The largest inputs are kept for the few cases that follow them only."""
    key = input_key(case, width)
    if key in _EXPECTED:
        _EXPECTED.move_to_end(key)
        return _EXPECTED[key]
    rels = build(case, width)
    srt = [np_sorted(width, t) for t in rels]
    for t in rels:
        t.setflags(write=False)
    for t in srt:
        t.setflags(write=False)
    cnt = np_count(*srt) if case.kind == "join" else None
    if case.kind == "join" and cnt < 10 ** 8:
        oc, oR, oS = orc.sortmergejoin(rels[0].copy(), rels[1].copy())
        assert oc == cnt
        assert np.array_equal(oR, srt[0]) and np.array_equal(oS, srt[1])
    elif case.kind == "sort":
        assert np.array_equal(orc.sort(rels[0]), srt[0])
    _EXPECTED[key] = (rels, srt, cnt)
    held = sum(sum(len(t) for t in v[0]) for v in _EXPECTED.values())
    while held > 12_000_000 and len(_EXPECTED) > 1:
        _, v = _EXPECTED.popitem(last=False)
        held -= sum(len(t) for t in v[0])
    return rels, srt, cnt


# ---------------------------------------------------------------------------
# the checks of every case
# ---------------------------------------------------------------------------
def _device_in(lib, t, off=0):
    """(arena, view): the relation on the device, `off` tuples into its arena
    (placement.arena); a valid pointer also when it is empty."""
    from placement import arena
    return arena(lib, len(t), off, fill=t)


def _device_out(lib, n, off=0):
    """(arena, view): n output tuples `off` tuples into an arena of
    sentinels, CANARY of them in front of the view and behind it."""
    from placement import arena
    return arena(lib, n, off)


def _check_out(lib, buf, view, want, what):
    from placement import check_guards
    check_guards(buf, view, f"{what}: output")
    assert np.array_equal(lib.to_host(view), want), f"{what}: sorted relation differs"


def run_case(lib, orc, case, placement=None, check=None):
    """The case (a join or a sort), twice on one fresh workspace, with all the
    checks of the module docstring.  placement: the tuple offsets of the
    buffers in their arenas, (R_in, S_in, R_out, S_out) for a join, (in, out)
    for a sort, or ("inplace", off) for a sort whose output is its input;
    None: all 0.  check(case, width, call, lib.skew_stats(), ran) is called
    after the checks of every call (ran: the traced kernels that ran)."""
    import torch
    from placement import check_guards
    width = lib.width
    if case.expect[width] is None:
        return "skip"
    rels, srt, cnt = expected(case, width, orc)
    k = len(rels)
    inplace = placement is not None and placement[0] == "inplace"
    if placement is None:
        placement = (0,) * (2 * k)
    elif inplace:
        assert case.kind == "sort"
        placement = (placement[1], placement[1])
    assert len(placement) == 2 * k
    lib.reset_workspace()
    lib.set_layouts(case.flags)
    try:
        ins = [_device_in(lib, t, off) for t, off in zip(rels, placement[:k])]
        for call in range(2):
            what = f"{case.name} w{width} call {call}"
            if inplace:
                if call:
                    ins = [_device_in(lib, t, off) for t, off in zip(rels, placement[:k])]
                outs = ins
            else:
                outs = [_device_out(lib, len(t), off) for t, off in zip(rels, placement[k:])]
            count = torch.full((1,), 0x7EADBEEF, dtype=torch.int64, device="cuda")
            lib.trace(True)
            if case.kind == "join":
                lo, hi = case.hint if case.hint is not None else (1, 0)
                lib.dev_join(ins[0][1], ins[1][1], outs[0][1], outs[1][1], count,
                             case.fanout, lo, hi)
            else:
                lib.dev_sort(ins[0][1], outs[0][1])
            torch.cuda.synchronize()
            trace = lib.trace_read()
            lib.trace(False)
            ran = {k for k, (_, launches) in trace.items() if launches > 0}
            if case.kind == "join":
                assert int(count.item()) == cnt, f"{what}: count {int(count.item())} != {cnt}"
            for (buf, view), t, name in zip(outs, srt, "RS"):
                _check_out(lib, buf, view, t, f"{what} {name}")
            if not inplace:
                for (buf, view), t, name in zip(ins, rels, "RS"):
                    assert np.array_equal(lib.to_host(view), t), f"{what}: input {name} changed"
                    check_guards(buf, view, f"{what}: input {name}")
            seen = (lib.last_layout(), "k_hist" in ran,
                    bool(ran & {"k_skew_small", "k_skew_hist"}))
            assert seen[0] == case.layout(width, call), f"{what}: layout {seen[0]}"
            assert seen[1] == case.exact(width, call), f"{what}: exact partition ran: {seen[1]}"
            if case.skew:
                assert seen[2], f"{what}: no skew kernel ran ({sorted(ran)})"
            if check is not None:
                check(case, width, call, lib.skew_stats(), ran)
    finally:
        lib.set_layouts(0)
        lib.reset_workspace()
    return "ran"


def run_cases(libs, oracles, width, cases, placement=None, check=None):
    done = [run_case(libs[width], oracles[width], c, placement, check) for c in cases]
    if "ran" not in done:
        pytest.skip(cases[0].why)


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("shapes", list(A_GROUPS))
@pytest.mark.parametrize("row", list(A_ROWS))
def test_forced_layout_by_shape(libs, oracles, width, row, shapes):
    """Group A: every layout, forced as the code allows, over the shapes."""
    run_cases(libs, oracles, width, group_a(row, A_GROUPS[shapes]))


@gpu
@pytest.mark.parametrize("case", A_FANOUT, ids=lambda c: c.name)
def test_fanout_past_sampled_scatter(libs, oracles, width, case):
    """Group A: D1 = 11 and 12 switch the sampled scatter off."""
    run_cases(libs, oracles, width, [case])


_B = group_b()


@gpu
@pytest.mark.parametrize("name", sorted({c.name.split("-")[1] for c in _B}))
def test_plan_edges(libs, oracles, width, name):
    """Group B: the usable() limits of the layouts and the 64-bit key range,
    through the join (hinted or not) and through the sort's guess."""
    run_cases(libs, oracles, width, [c for c in _B if c.name.split("-")[1] == name])


@gpu
@pytest.mark.parametrize("row", list(C_ROWS))
def test_sort_small_sizes_by_layout(libs, oracles, width, row):
    """Group C: small and ragged sorts in every layout."""
    run_cases(libs, oracles, width, group_c(row))


@gpu
@pytest.mark.parametrize("row", list(D_ROWS))
def test_fused_count_above_2_32(libs, oracles, width, row):
    """Group D: 70 000 (and 392 216) copies of one key on both sides, payloads
    shuffled: the count of k_groupsort and the skew kernels passes 2^32."""
    cases = group_d(row)
    for c in cases:
        if c.expect[width] is not None:
            _, _, cnt = expected(c, width, oracles[width])
            copies = c.nR - 1000
            assert cnt == (copies + 1) ** 2 + 999 and cnt > 1 << 32
    run_cases(libs, oracles, width, cases)
