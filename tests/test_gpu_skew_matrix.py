"""The group pass's queue and the skew path, case by case.

A group that k_groupsort (bucketsort.hip) cannot finish in LDS is queued
(group_overflow), the host splits the queue at kSkewSmall (skew_path),
k_skew_small or k_skew_hist/_scan/_place/_check sort and count it on the
device, and what they flag goes back through segmented_sort and
merge_join_count_batch.  The layout matrix reaches that chain with one hot key
in one large group only.  The cases below walk it: equal-digit runs at
GS_RUNMAX, groups at GS_CAP and kSkewSmall, large groups of many keys, work
items up to their cap, inexact digits, buckets of more tiles than the group
pass's tables hold (TPL 2 and 4, the run-by-run branch past SK_TM) and queued
groups between unqueued ones in pair mode.

Every case runs through test_gpu_layout_matrix.run_case (sorted relations and
count bit-exact against numpy, guards, inputs, second call, layout), and on
top of it compares smj_workspace_skew_stats with predict(): the record that
the restated plan and the generated keys give, never one read from the
library.  Where the record depends on the order in which the device happens to
place equal keys, predict() gives a bound and says so:

* The placement orders of the group pass and of the skew kernels do not look
  at the payloads, which are random here: the d distinct tuples of one key come
  out in (key, payload) order with probability 1/d! <= 2^-(d-1).  A run of more
  than GS_RUNMAX equal digits that holds 21 or more distinct tuples is
  therefore taken to fail in the group pass (1/21! < 2^-64; the table holds no
  run with 2 to 20, predict() refuses one), and a queued group whose keys sum
  to 64 or more of (distinct tuples - 1) is taken to come out of the skew
  kernels with an inversion (flag bit 1).  With a sum of 1 to 63 the group may
  or may not be flagged: `unordered` and `resorted` are then bounds.

Deviation from the issue's pair-mode shape: "every third group hot, 3000 and
20 000 tuples alternately" needs 5198 tuples a group on average, and a sort
whose size guess holds plans 2048 a group.  The hot groups are every third
of the first 48 (45) groups; the others share the rest of the tuples.
"""
import collections

import numpy as np
import pytest

import test_gpu_layout_matrix as M
from test_gpu_layout_matrix import Case, expected, choose_levels, make_plan, NO_SAMPLED

# ---------------------------------------------------------------------------
# the constants of bucketsort.hip, restated (test_skew_restatement pins them)
# ---------------------------------------------------------------------------
GS_CAP = 2560          # line 176: GS_THREADS * GS_ITEMS, tuples a group a relation
GS_RUNMAX = 32         # line 184: longest equal-digit run fixed serially
GS_NB3 = 1 << 11       # line 179
K_SKEW_SMALL = 16384   # line 1751: SK_THREADS * 64
SKEW_ITEM = 8192       # line 1753: SMJ_SKEW_ITEM
SKEW_ITEM_CAP = 256    # skew_path: ts = min(max(nr / SMJ_SKEW_ITEM, 1), 256)
SK_TM = 256            # line 1755: tile runs in k_skew_small's LDS tables
SHARDS = 8             # smj_internal.hpp kShards: segments of a sampled partition's bucket
U = 393_216            # 8 x 49 152: every layout's scatter tiles, all shards level


def tile_elems(layout, width):
    """tile_elems_l<Lay>() (bucketsort.hip lines 97-123): TP_THREADS (1024) x
    tp_items<W>, the 128 KB stage over sizeof(W) (64 KB for 4-byte words, which
    makes 16384 too; the 48-bit planes keep the tile of 8-byte elements).
    12-byte elements: 131072 / 12 = 10922, / 1024 = 10 a thread."""
    if layout == "p96":
        return 10240
    if layout == "tuples" and width == 16:
        return 8192
    return 16384


def expected_tiles(nmax, nb, nseg, tsz):
    """expected_tiles (bucketsort.hip, in front of group_tpl)."""
    per = nmax // max(nb, 1)
    return (per + per // 4) // tsz + nseg + 1


def group_tpl(nmax, nb, nseg, tsz):
    return 2 if expected_tiles(nmax, nb, nseg, tsz) <= 128 else 4


def skew_items(nr):
    return min(max(nr // SKEW_ITEM, 1), SKEW_ITEM_CAP)


# the rows of the layout matrix that apply: (flags, payloads, layout at 8 / 16)
ROWS = {r: M.A_ROWS[r] for r in ("p32", "p48", "words", "p96", "tuples_sampled", "tuples_exact")}


class SkewCase(Case):
    """A case of the layout matrix with its claims about the record:
    claims[width] (or claims[None] for both) = {field: value}, checked against
    predict() on the CPU, and `totals`, the (R, S) size of the hot group."""

    def __init__(self, name, kind, nR, nS, fanout, row, hint, keys, claims=None, fix=None,
                 totals=None, pay=None, widths=(8, 16), group="", runs=None, tiles=None,
                 fits=False):
        flags, rpay, _, e8, e16 = ROWS[row]
        expect = {8: e8 if 8 in widths else None, 16: e16 if 16 in widths else None}
        Case.__init__(self, name, kind, nR, nS, fanout, flags, hint, keys, pay or rpay, expect,
                      why="no such layout or case at this width")
        self.row, self.claims, self.fix, self.totals = row, claims or {}, fix, totals
        self.group, self.runs, self.tiles, self.fits = group, runs, tiles, fits

    def plan(self, width):
        """16-byte tuples in their own layout or as 12-byte elements choose the
        level widths again for tiles of 8192 (capi.hip tuple_plan)."""
        lo, hi = self.plan_range(width)
        nmax = max(self.ns)
        lv = choose_levels(nmax, self.fanout)
        if width == 16 and self.expect[16] and self.layout(16) in ("tuples", "p96"):
            lt = choose_levels(nmax, self.fanout, M.K_TILE_TUPLES // 2)
            sampled = not (self.flags & NO_SAMPLED) and lv[1] <= 10
            if lt[1] != lv[1] and not (sampled and lt[1] > 10):
                lv = lt
        return make_plan(lo, hi, lv)

    def claim(self, width):
        return {**self.claims.get(None, {}), **self.claims.get(width, {})}


# ---------------------------------------------------------------------------
# the record, predicted from the restated plan and the generated keys
# ---------------------------------------------------------------------------
Pred = collections.namedtuple("Pred", "stats cnt queued tiles_lo tiles_hi plan tpl runmax")
_PRED = {}


def _groups_of(keys, p):
    """(group, level-3 digit prefix, clamped) of every key under plan p; both
    digits rise with the key."""
    k = np.asarray(keys, np.int64)
    rel = k.astype(np.uint64) - np.uint64(p.base % (1 << 64))  # mod 2^64, as key_u
    below = k < p.base
    above = ~below & (rel > np.uint64(p.span))
    rel = np.where(below, np.uint64(0), np.where(above, np.uint64(p.span), rel))
    return (rel >> np.uint64(p.s2)).astype(np.int64), rel >> np.uint64(p.s3), below | above


def _runs(ids, ks, ps, longer_than=GS_RUNMAX, sample=128):
    """The runs of equal `ids` in relations sorted by key (ks, ps: keys and
    payloads): (start, length, alike, distinct) of every run.  alike: all its
    tuples are one; distinct: a lower bound of its distinct tuples, 2 for a run
    that is not alike, and for a run of more than `longer_than` tuples the
    distinct ones among its first `sample`."""
    n = len(ids)
    start = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]]) if n else np.zeros(0, np.int64)
    length = np.diff(np.r_[start, n])
    if not n:
        return start, length, np.zeros(0, bool), np.zeros(0, np.int64)
    alike = (np.minimum.reduceat(ps, start) == np.maximum.reduceat(ps, start)) & \
            (ks[start] == ks[start + length - 1])
    distinct = np.where(alike, 1, 2)
    sel = np.flatnonzero((length > longer_than) & ~alike)
    if len(sel):
        m = np.minimum(length[sel], sample)
        run = np.repeat(np.arange(len(sel)), m)
        first = np.cumsum(m) - m
        idx = start[sel][run] + (np.arange(int(m.sum())) - first[run])
        o = np.lexsort((ps[idx], ks[idx], run))
        kk, pp, rr = ks[idx][o], ps[idx][o], run[o]
        new = np.r_[True, (rr[1:] != rr[:-1]) | (kk[1:] != kk[:-1]) | (pp[1:] != pp[:-1])]
        distinct[sel] = np.add.reduceat(new.astype(np.int64), first)
    return start, length, alike, distinct


def predict(case, width, call=0, rels=None):
    """The smj_skew_stats of the case as {field: (lowest, highest)}."""
    lay, exact_part = case.layout(width, call), case.exact(width, call)
    key = (M.input_key(case, width), case.hint, case.fanout, lay, exact_part)
    if key in _PRED:
        return _PRED[key]
    if rels is None:
        rels = M.build(case, width)
    p = case.plan(width)
    nrel = len(rels)
    tsz = tile_elems(lay, width)
    nseg = 1 if exact_part else SHARDS
    nb, nb2 = 1 << p.D1, 1 << p.D2
    ng = nb * nb2
    tpl = group_tpl(max(case.ns), nb, nseg, tsz)
    cnt = np.zeros((2, ng), np.int64)
    fails = np.zeros(ng, bool)       # a long equal-digit run of 21 or more distinct tuples
    may_fail = np.zeros(ng, bool)    # ... of 2 to 20, as far as counted
    clamped = np.zeros(ng, bool)
    differ = np.zeros(ng, np.int64)  # sum over the keys of (distinct tuples - 1), at least
    over = np.zeros(nb, bool)
    tiles_lo, tiles_hi, runmax = [], [], []
    for r, t in enumerate(rels):
        order = np.argsort(t["key"])
        ks, ps = t["key"][order].astype(np.int64), t["payload"][order]
        gid, d3, cl = _groups_of(ks, p)
        cnt[r] = np.bincount(gid, minlength=ng)
        clamped[np.unique(gid[cl])] = True
        # equal-digit runs past GS_RUNMAX: in order with 1 / 21! < 2^-64 from 21 distinct tuples
        start, length, alike, distinct = _runs(d3, ks, ps)
        runmax.append(int(length.max()) if len(length) else 0)
        long_run = length > GS_RUNMAX
        fails[gid[start[long_run & (distinct >= 21)]]] = True
        may_fail[gid[start[long_run & ~alike & (distinct < 21)]]] = True
        # d distinct tuples of a key come out in order with 1 / d! <= 2^-(d - 1)
        if p.s3 or cl.any():   # (else a digit is a key)
            start, length, alike, distinct = _runs(ks, ks, ps)
        differ += np.bincount(gid[start], weights=distinct - 1, minlength=ng).astype(np.int64)
        # tiles of every bucket: its segments' tiles, each rounded up
        bc = cnt[r].reshape(nb, nb2).sum(axis=1)
        lo = (bc + tsz - 1) // tsz
        hi = lo if exact_part else np.where(bc > 0, bc // tsz + nseg, 0)
        tiles_lo.append(lo)
        tiles_hi.append(hi)
        assert not ((lo <= 64 * tpl) & (hi > 64 * tpl)).any(), \
            f"{case.name} w{width}: a bucket that may or may not pass {64 * tpl} tiles"
        over |= lo > 64 * tpl
    fit = (cnt[0] <= GS_CAP) & (cnt[1] <= GS_CAP)
    queued = np.repeat(over, nb2) | ~fit | fails
    assert not (may_fail & ~queued).any(), f"{case.name} w{width}: a run that may or may not fail"
    m = cnt.max(axis=0)
    small = queued & (m <= K_SKEW_SMALL)
    large = queued & ~small
    items = sum(skew_items(int(cnt[r][g])) for g in np.flatnonzero(large) for r in range(nrel))
    inexact = queued & (clamped | (p.s3 != 0))
    ex = queued & ~inexact
    un_lo, un_hi = int((ex & (differ >= 64)).sum()), int((ex & (differ >= 1)).sum())
    nin = int(inexact.sum())
    both = (cnt[0] > 0) & (cnt[1] > 0) if nrel == 2 else np.zeros(ng, bool)

    def one(v):
        return (int(v), int(v))
    stats = {"tpl": one(tpl), "queued": one(queued.sum()), "empty": one((queued & (m == 0)).sum()),
             "small": one(small.sum()), "large": one(large.sum()), "items": one(items),
             "inexact": one(nin), "unordered": (un_lo, un_hi),
             "resorted": (nin + un_lo, nin + un_hi), "recounted": one((inexact & both).sum())}
    out = Pred(stats, cnt, queued, tiles_lo, tiles_hi, p, tpl, runmax)
    if len(_PRED) > 64:
        _PRED.clear()
    _PRED[key] = out
    return out


def check_record(case, width, call, stats, ran):
    """run_case's hook: the record of this call against predict()."""
    what = f"{case.name} w{width} call {call}"
    pred = predict(case, width, call, expected(case, width, None)[0])
    assert stats is not None, f"{what}: no record"
    print(f"{what}: {stats}")
    for name, (lo, hi) in pred.stats.items():
        assert lo <= stats[name] <= hi, f"{what}: {name} {stats[name]} not in [{lo}, {hi}]: {stats}"
    assert ("k_skew_small" in ran) == (pred.stats["small"][0] > 0), f"{what}: {sorted(ran)}"
    assert ("k_skew_hist" in ran) == (pred.stats["large"][0] > 0), f"{what}: {sorted(ran)}"


# ---------------------------------------------------------------------------
# key generators: f(rng, width, nR[, nS]) -> key arrays, as in the layout matrix
# ---------------------------------------------------------------------------
def _tagged(f, tag):
    f.tag = tag
    return f


def _spread(rng, lo, hi, n, without=None):
    """n uniform keys in [lo, hi], none in the range `without`."""
    k = rng.integers(lo, hi, n, dtype=np.int64, endpoint=True)
    while without is not None:
        bad = (k >= without[0]) & (k <= without[1])
        if not bad.any():
            break
        k[bad] = rng.integers(lo, hi, int(bad.sum()), dtype=np.int64, endpoint=True)
    return k


def _distinct_outside(rng, lo, hi, n, without):
    """n keys of [lo, hi] outside `without`: distinct as far as there are that
    many (dense ranges), the rest (or all, in a wide range) uniform draws."""
    if hi - lo < 1 << 24:
        pool = np.concatenate([np.arange(lo, without[0], dtype=np.int64),
                               np.arange(without[1] + 1, hi + 1, dtype=np.int64)])
        k = rng.permutation(pool)[:n]
        return np.concatenate([k, _spread(rng, lo, hi, n - len(k), without)])
    return _spread(rng, lo, hi, n, without)


def hot_gid(case, width):
    """The group hot_group() fills: the middle one of the hinted key range."""
    p = case.plan(width)
    return ((case.hint[1] - p.base + 1) >> p.s2) // 2


def hot_group(case, tR, tS, hotR=True):
    """One hot key in the middle group of the plan's populated key range
    [lo, hi] = the hint: relation r holds exactly t_r tuples of that group's
    2^s2 keys, min(t_r / 2, 1000) of them distinct other keys and the rest the
    hot key (hotR false: R holds t_R other keys and no hot one); every key
    outside the group at most a few times."""
    def f(rng, width, nR, nS):
        p = case.plan(width)
        lo, hi = case.hint
        gk = 1 << p.s2
        g0 = p.base + hot_gid(case, width) * gk
        hot = g0 + gk // 2
        out, outside_r = [], None
        for n, t, has_hot in ((nR, tR, hotR), (nS, tS, True)):
            others = min(t // 2, 1000) if has_hot else t
            assert others < gk // 2
            step = (gk // 2 - 1) // max(others, 1)
            ko = g0 + np.arange(others, dtype=np.int64) * step  # below the hot key, distinct
            kh = np.full(t - others, hot, np.int64)
            kout = _distinct_outside(rng, lo, hi, n - t, (g0, g0 + gk - 1))
            if outside_r is not None and hi - lo >= 1 << 24:
                # a wide range: half of S's other tuples repeat keys of R
                kout[: len(kout) // 2] = rng.choice(outside_r, len(kout) // 2)
            outside_r = kout if outside_r is None else outside_r
            out.append(rng.permutation(np.concatenate([ko, kh, kout])))
        return out
    return _tagged(f, f"hotgroup{tR}:{tS}:{int(hotR)}:{case.hint}:{case.fanout}:{case.row}")


def run_keys(c):
    """Every key c times a relation, the keys n // c steps of n // (n // c)
    apart from 1 (so that a group of 2048 keys stays below GS_CAP); what is left
    of n as copies of the key n."""
    def f(rng, width, nR, nS=None):
        out = []
        for n in (nR,) if nS is None else (nR, nS):
            nk = n // c
            k = np.repeat(1 + np.arange(nk, dtype=np.int64) * (n // nk), c)
            out.append(rng.permutation(np.concatenate([k, np.full(n - nk * c, n, np.int64)])))
        return out
    return _tagged(f, f"runs{c}")


def cluster_keys(c, shift):
    """2048 consecutive keys c times each on both sides, from the start of a
    group's key range (+ shift), the rest distinct keys of 1..n."""
    def f(rng, width, nR, nS):
        k0 = 1 + 2048 * ((nR // 2048) // 2) + shift
        out = []
        for n in (nR, nS):
            k = np.repeat(np.arange(k0, k0 + 2048, dtype=np.int64), c)
            rest = _distinct_outside(rng, 1, n, n - len(k), (k0, k0 + 2047))
            out.append(rng.permutation(np.concatenate([k, rest])))
        return out
    return _tagged(f, f"cluster{c}:{shift}")


def heavy_bucket(low_hi, high_hi, n_high, skip_every=0):
    """R: nR - n_high keys uniform in 1..low_hi (skip_every: none in every
    skip_every-th range of 2048 keys), n_high in low_hi+1..high_hi; S: nS draws
    from R's keys."""
    def f(rng, width, nR, nS):
        k = rng.integers(1, low_hi, nR - n_high, dtype=np.int64, endpoint=True)
        if skip_every:
            while True:
                bad = ((k - 1) >> 11) % skip_every == skip_every - 1
                if not bad.any():
                    break
                k[bad] = rng.integers(1, low_hi, int(bad.sum()), dtype=np.int64, endpoint=True)
        kR = np.concatenate([k, rng.integers(low_hi + 1, high_hi, n_high, dtype=np.int64,
                                             endpoint=True)])
        kR = rng.permutation(kR)
        return [kR, kR[rng.integers(0, nR, nS)]]
    return _tagged(f, f"heavy{low_hi}:{high_hi}:{n_high}:{skip_every}")


def uniform_keys(hi):
    def f(rng, width, nR, nS):
        kR = rng.integers(1, hi, nR, dtype=np.int64, endpoint=True)
        return [kR, kR[rng.integers(0, nR, nS)]]
    return _tagged(f, f"uniform{hi}")


def pair_keys(ngroups, nhot):
    """A sort's keys in 1..n: the groups 0, 3, 6, .. (nhot of them) hold one key
    each, 3000 and 20 000 times alternately; the other groups of the first
    `ngroups` share the rest as uniform draws of their 2048-key ranges."""
    def f(rng, width, nR, nS=None):
        hot = 3 * np.arange(nhot)
        ks = [np.full(3000 if i % 2 == 0 else 20_000, 1 + 2048 * g + 1000, np.int64)
              for i, g in enumerate(hot)]
        rest = nR - sum(len(k) for k in ks)
        others = np.setdiff1d(np.arange(ngroups), hot)
        g = others[np.arange(rest) % len(others)]
        ks.append(1 + 2048 * g + rng.integers(0, 2048, rest))
        return [rng.permutation(np.concatenate(ks))]
    return _tagged(f, f"pair{ngroups}:{nhot}")


def clamp_keys(inside_hi, n_out, hot_copies):
    """Keys uniform in 1..inside_hi (the hint), and n_out tuples above it:
    hot_copies of one key, the others distinct."""
    def f(rng, width, nR, nS):
        out = []
        for n in (nR, nS):
            k_out = np.concatenate([np.full(hot_copies, inside_hi + 40_000, np.int64),
                                    inside_hi + 1 + np.arange(n_out - hot_copies, dtype=np.int64)])
            k = rng.integers(1, inside_hi, n - n_out, dtype=np.int64, endpoint=True)
            out.append(rng.permutation(np.concatenate([k, k_out])))
        return out
    return _tagged(f, f"clamp{inside_hi}:{n_out}:{hot_copies}")


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def _widths(row):
    return tuple(w for w, e in ((8, ROWS[row][3]), (16, ROWS[row][4])) if e is not None)


# ---- R: equal-digit runs at GS_RUNMAX (U tuples a side: D1 = 8, s2 = 11, s3 = 0)
def group_r(row):
    out = []
    for kind in ("join", "sort"):
        if kind == "sort" and row == "tuples_exact":
            continue    # no size guess without the sampled scatter: the sort's own plan
        hint = (1, U) if kind == "join" else None
        fan = 8 if kind == "join" else 0
        for c, fix, claims in (
                (32, None, {"queued": 0}),
                (33, "ident", {"queued": 0}),
                # every populated group holds runs of 33 differing tuples (the
                # bound of the module docstring: 1/33! a run)
                (33, None, {"queued": 192, "small": 192, "unordered": 192, "resorted": 192,
                            "recounted": 0, "empty": 0})):
            out.append(SkewCase(f"R-{row}-{kind}-{c}{'i' if fix else ''}", kind, U, U, fan, row, hint,
                                run_keys(c), {None: claims}, fix=fix, group="R", runs=c))
    return out


# ---- Z: one hot key, the group's size at GS_CAP and kSkewSmall
Z_SIZES = [
    # name, (R, S) tuples of the hot group, hot key in R, claims
    ("cap", (2560, 2560), True, None),   # queued 0 only with identical hot tuples (below)
    ("cap+1_r", (2561, 100), True, {"queued": 1, "small": 1}),
    ("cap+1_s", (100, 2561), True, {"queued": 1, "small": 1}),
    ("cap+1_s0", (2561, 0), True, {"queued": 1, "small": 1}),   # nr[1] == 0
    ("small", (16384, 16384), True, {"queued": 1, "small": 1}),
    ("small+1_r", (16385, 200), True, {"queued": 1, "large": 1, "items": 2 + 1}),
    ("small+1_s", (200, 16385), True, {"queued": 1, "large": 1, "items": 1 + 2}),
    ("items", (40960, 24576), True, {"queued": 1, "large": 1, "items": 5 + 3}),
    ("absent", (100, 2561), False, {"queued": 1, "small": 1}),  # hot key in S only
]


def group_z(row, fix, n=U, fan=8, sizes=None):
    out = []
    for name, tot, hot_r, claims in Z_SIZES:
        if sizes and name not in sizes:
            continue
        claims = dict(claims or {})
        if name == "cap":
            # 1560 equal digits: in order only when the tuples are all alike
            claims = {"queued": 0} if fix else {"queued": 1, "small": 1}
        if claims["queued"]:
            un = 0 if fix else 1
            claims.update(unordered=un, resorted=un, recounted=0, inexact=0)
        c = SkewCase(f"Z-{row}-{name}-{n}-{fix or 'shuffled'}", "join", n, n, fan, row, (1, n), None,
                     {None: claims}, fix=fix, totals=tot, group="Z")
        c.keys = hot_group(c, tot[0], tot[1], hot_r)
        out.append(c)
    return out


# 1 050 000 x 1 050 000 at fan-out 1 under the 48-bit planes: D2 = 9, the
# 16-byte library's tile pass writes LayP40
def z_p40():
    return [c for fix in (None, "ident")
            for c in group_z("p48", fix, 1_050_000, 1, ("cap+1_r", "small", "items"))]


# ---- K: 2048 keys in one queued group (or 1024 in each of two)
K_CASES = [
    # copies, n, shift, claims
    (3, U, 0, {"queued": 1, "small": 1}),
    (3, U, 1024, {"queued": 2, "small": 2}),
    (10, U, 0, {"queued": 1, "large": 1, "items": 2 + 2}),
    (10, U, 1024, {"queued": 2, "small": 2}),        # 10 240 + its other keys a group
    # 2 252 800 tuples in a bucket planned for 9216 (TPL 2): 137 tiles and more,
    # so the bucket's eight groups are queued, the cluster's among them; the
    # others hold distinct keys
    (1100, 6 * U, 0, {"queued": 8, "small": 7, "large": 1, "items": 256 + 256, "unordered": 1}),
    (1100, 6 * U, 1024, {"queued": 8, "small": 6, "large": 2, "items": 4 * 137, "unordered": 2}),
]


def group_k(row):
    out = []
    for c, n, shift, claims in K_CASES:
        q = claims.get("unordered", claims["queued"])
        claims = dict(claims, unordered=q, resorted=q, recounted=0, inexact=0)
        out.append(SkewCase(f"K-{row}-{c}-{shift}", "join", n, n, 8, row, (1, n),
                            cluster_keys(c, shift), {None: claims}, group="K"))
    return out


# ---- E: inexact digits
def group_e(row):
    out = []
    wide = {8: (M.I32_MIN, M.I32_MAX), 16: (-(1 << 62), (1 << 62) - 1)}
    for name, tot, claims in (("small", (2561, 100), {"small": 1}),
                              ("large", (16385, 200), {"large": 1, "items": 3})):
        claims = dict(claims, queued=1, inexact=1, resorted=1, recounted=1, unordered=0)
        for w in (8, 16):
            # (a) key bits below the last digit: s3 = 11 (8 bytes), 42 (16)
            c = SkewCase(f"E-{row}-s3-{name}-w{w}", "join", U, U, 8, row, wide[w], None,
                         {None: claims}, totals=tot, widths=(w,), group="Ea")
            c.keys = hot_group(c, tot[0], tot[1])
            out.append(c)
    # (b) the hint 1..2^18 and 3000 / 20 000 tuples above it: they clamp to the
    # last group's digit (1024 keys, about 1500 tuples of its own)
    for name, n_out, hot, claims in (("small", 3000, 2000, {"small": 1}),
                                     ("large", 20_000, 17_000, {"large": 1, "items": 2 + 2})):
        claims = dict(claims, queued=1, inexact=1, resorted=1, recounted=1, unordered=0)
        c = SkewCase(f"E-{row}-clamp-{name}", "join", U, U, 8, row, (1, 1 << 18),
                     clamp_keys(1 << 18, n_out, hot), {None: claims}, group="Eb")
        out.append(c)
    return out


# ---- T: buckets of more tiles than the group pass's tables hold (fan-out 1)
def group_t():
    t16 = {"widths": (16,)}
    over8 = heavy_bucket(1 << 21, 1 << 22, 150_000)
    return [
        # bucket 0: >= 139 tiles of 8192 > 128, every one of its 512 groups queued
        SkewCase("T-over-16t", "join", 3 * U, U, 1, "tuples_sampled", (1, 1 << 21),
                 heavy_bucket(1 << 20, 1 << 21, 40_000),
                 {None: {"tpl": 2, "queued": 512, "small": 512, "empty": 0}},
                 tiles=(139, 128), group="T", fits=True, **t16),
        SkewCase("T-over-8", "join", 6 * U, U, 1, "p48", (1, 1 << 22), over8,
                 {None: {"tpl": 2, "queued": 1024, "small": 1024, "empty": 0}},
                 tiles=(134, 128), group="T", fits=True),
        SkewCase("T-over-8-p32", "join", 6 * U, U, 1, "p32", (1, 1 << 22), over8,
                 {None: {"tpl": 2, "queued": 1024, "small": 1024, "empty": 0}},
                 pay="bit", tiles=(134, 128), group="T", fits=True),
        SkewCase("T-over-empty", "join", 3 * U, U, 1, "tuples_sampled", (1, 1 << 21),
                 heavy_bucket(1 << 20, 1 << 21, 40_000, skip_every=4),
                 {None: {"tpl": 2, "queued": 512, "small": 512, "empty": 128}},
                 tiles=(139, 128), group="T", **t16),
        # > SK_TM tiles: k_skew_small goes run by run
        SkewCase("T-runs-16t", "join", 6 * U, U, 1, "tuples_sampled", (1, 1 << 22), over8,
                 {None: {"tpl": 4, "queued": 1024, "small": 1024, "empty": 0}},
                 tiles=(269, SK_TM), group="T", fits=True, **t16),
        SkewCase("T-runs-8", "join", 12 * U, U, 1, "p48", (1, 1 << 22),
                 heavy_bucket(1 << 21, 1 << 22, 200_000),
                 {None: {"tpl": 4, "queued": 1024, "small": 1024, "empty": 0}},
                 tiles=(275, SK_TM), group="T"),
    ] + [
        # TPL 4 with every group in LDS: two buckets of 132 tiles (12-byte
        # elements: tuple_plan makes it four buckets of 10240-element tiles)
        SkewCase(f"T-tpl4-{row}", "join", 11 * U, U, 1, row, (1, 1 << 22), uniform_keys(1 << 22),
                 {None: {"tpl": 4, "queued": 0}}, widths=w, group="T4")
        for row, w in (("p48", (8, 16)), ("words", (16,)), ("p96", (16,)), ("tuples_sampled", (8,)))
    ]


# ---- P: pair mode, queued slots between unqueued ones
def group_p(row):
    return [SkewCase(f"P-{row}-{ng}", "sort", U, U, 0, row, None, pair_keys(ng, nhot),
                     {None: {"queued": nhot, "small": (nhot + 1) // 2, "large": nhot // 2,
                             "items": 2 * (nhot // 2), "unordered": nhot, "resorted": nhot,
                             "recounted": 0, "inexact": 0}}, group="P")
            for ng, nhot in ((192, 16), (191, 15))]


Z_ROWS = list(ROWS)
R_ROWS = ["p32", "p48", "tuples_sampled", "tuples_exact"]
K_ROWS = ["p48", "words", "p96", "tuples_sampled"]
E_ROWS = ["tuples_sampled", "tuples_exact"]
P_ROWS = ["p32", "p48", "tuples_sampled"]


def all_cases():
    out = []
    for row in R_ROWS:
        out += group_r(row)
    for row in Z_ROWS:
        out += group_z(row, None) + group_z(row, "ident")
    out += z_p40()
    for row in K_ROWS:
        out += group_k(row)
    for row in E_ROWS:
        out += group_e(row)
    out += group_t()
    for row in P_ROWS:
        out += group_p(row)
    return out


# ---------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------
def test_skew_restatement():
    """The restated tile sizes, TPL choice and work items against the source's
    own comments: tiles of 16384 8-byte elements, 8192 16-byte tuples ("a bucket
    of up to 3.1M of them is 384 tiles"), ten 12-byte elements a thread; 128
    tiles at TPL 2; a 40 960-tuple relation in 5 work items, 2 097 152 in 256."""
    assert [tile_elems(lay, 8) for lay in ("p32", "p48", "tuples")] == [16384] * 3
    assert [tile_elems(lay, 16) for lay in ("p32", "p48", "words", "p96", "tuples")] == \
        [16384, 16384, 16384, 10240, 8192]
    assert 3_145_728 // tile_elems("tuples", 16) == 384
    assert (128 * 1024 // 12) // 1024 * 1024 == tile_elems("p96", 16)
    assert GS_CAP * 4 // 5 == M.K_GROUP_TARGET and GS_NB3 == 1 << M.K_GROUP_D3MAX
    assert K_SKEW_SMALL == 256 * 64
    # mean bucket + 1/4 in tiles, a partial tile a segment, one more
    assert expected_tiles(1 << 27, 256, SHARDS, 16384) == 40 + 9
    assert group_tpl(6 * U, 2, SHARDS, 16384) == 2 and expected_tiles(6 * U, 2, SHARDS, 16384) == 99
    assert group_tpl(11 * U, 2, SHARDS, 16384) == 4
    assert group_tpl(6 * U, 2, SHARDS, 8192) == 4 and group_tpl(3 * U, 2, SHARDS, 8192) == 2
    assert [skew_items(n) for n in (0, 8191, 16385, 24576, 40960, 2_097_151, 2_097_152, 1 << 30)] == \
        [1, 1, 2, 3, 5, 255, 256, 256]
    # tuple_plan: 11 U tuples at fan-out 1 are two buckets of 8-byte elements, four of 16-byte ones
    assert choose_levels(11 * U, 1)[1] == 1 and choose_levels(11 * U, 1, 8192)[1] == 2
    assert choose_levels(6 * U, 1, 8192)[1] == 1


def test_skew_fields_match_binding():
    import smj
    assert smj.SKEW_STATS == ("tpl", "queued", "empty", "small", "large", "items", "inexact",
                              "unordered", "resorted", "recounted")
    assert "smj_workspace_skew_stats" in smj.DEVICE_SYMBOLS


def _case_holds(c, w):
    """One case at one width holds what it claims under the restated plan and
    its generated keys: layout conditions, the record, the hot group's totals,
    run lengths, tile counts, the fit condition."""
    p = c.plan(w)
    lay = c.layout(w)
    if c.kind == "join":
        assert M.layout_usable(lay, w, p, c.flags, True), (c.name, w, lay, p)
    if lay in M.WORD_BITS:
        assert c.pay_bits(w) <= M.WORD_BITS[lay] - p.s1, (c.name, w)
    rels = M.build(c, w)
    assert [len(t) for t in rels] == list(c.ns), c.name
    if c.kind == "sort":   # the size guess 1..n holds
        assert rels[0]["key"].min() >= 1 and rels[0]["key"].max() <= c.nR, c.name
    pr = predict(c, w, 0, rels)
    st = pr.stats
    for name, v in c.claim(w).items():
        assert st[name] == (v, v), (c.name, w, name, st[name], v)
    q = np.flatnonzero(pr.queued)
    if c.totals:
        assert tuple(pr.cnt[:, hot_gid(c, w)]) == c.totals, (c.name, w)
        assert set(q) <= {hot_gid(c, w)}, (c.name, w, q)
    if c.runs:
        assert pr.runmax == [c.runs] * len(rels), (c.name, pr.runmax)
    if c.group in ("R", "T4") or c.fits:
        # the groups fit: only the run length or the tile count queues them
        assert pr.cnt.max() <= GS_CAP, (c.name, w, pr.cnt.max())
    if c.tiles:
        at_least, more_than = c.tiles
        assert pr.tiles_lo[0][0] >= at_least > more_than >= 64 * pr.tpl, (c.name, w, pr.tiles_lo[0])
        assert pr.tiles_hi[0][1:].max() <= 64 * pr.tpl and pr.tiles_hi[1].max() <= 64 * pr.tpl
        if more_than < SK_TM:
            assert pr.tiles_hi[0][0] <= SK_TM, c.name
        assert pr.cnt.max() <= K_SKEW_SMALL
    if c.group == "T4":
        assert pr.tpl == 4 and max(h.max() for h in pr.tiles_hi) <= 64 * 4, c.name
    if c.group == "Ea":
        assert p.s3 > 0, (c.name, w)
    if c.group == "Eb":
        assert p.s3 == 0 and st["inexact"] == (1, 1), (c.name, w)
    if c.group == "P":
        assert {int(g) % 2 for g in q} == {0, 1}, c.name    # queued groups in both slots of a pair
        assert not pr.queued[q + 1].any() and not pr.queued[q[1:] - 1].any(), c.name
        assert len(np.flatnonzero(pr.cnt[0])) == int(c.name.split("-")[-1]), c.name


CPU_GROUPS = {**{f"R-{row}": (group_r, row) for row in R_ROWS},
              **{f"Z-{row}-{fix or 'shuffled'}": (group_z, row, fix)
                 for row in Z_ROWS for fix in (None, "ident")},
              "Z-p40": (z_p40,),
              **{f"K-{row}": (group_k, row) for row in K_ROWS},
              **{f"E-{row}": (group_e, row) for row in E_ROWS},
              "T": (group_t,),
              **{f"P-{row}": (group_p, row) for row in P_ROWS}}


@pytest.mark.parametrize("group", list(CPU_GROUPS))
def test_skew_cases_hold_their_claims(group):
    f, *args = CPU_GROUPS[group]
    for c in f(*args):
        for w in (8, 16):
            if c.expect[w] is not None:
                _case_holds(c, w)


def test_skew_table_reaches_edges():
    """The table as a whole (its claims, which test_skew_cases_hold_their_claims
    checks case by case) reaches the edges the queue and the skew path have."""
    cases = all_cases()
    assert sorted(c.name for c in cases) == sorted(c.name for f, *a in CPU_GROUPS.values() for c in f(*a))
    assert len({c.name for c in cases}) == len(cases)
    claims = [(c, w, c.claim(w)) for c in cases for w in (8, 16) if c.expect[w] is not None]
    assert {w for _, w, _ in claims} == {8, 16}
    totals = {t for c in cases if c.totals for t in c.totals}
    assert {GS_CAP, GS_CAP + 1, K_SKEW_SMALL, K_SKEW_SMALL + 1, 0} <= totals
    for big, little in ((GS_CAP + 1, 100), (K_SKEW_SMALL + 1, 200)):   # one over, the other under
        assert {(big, little), (little, big)} <= {c.totals for c in cases}
    per_relation = {skew_items(t) for t in totals if t > 0} | {skew_items(2048 * c[0]) for c in K_CASES}
    assert {1, 2, 5, SKEW_ITEM_CAP} <= per_relation
    assert 2048 * 1100 >= SKEW_ITEM * SKEW_ITEM_CAP
    assert {cl.get("tpl") for _, _, cl in claims} >= {2, 4}
    tiles = {c.tiles[1] for c in cases if c.tiles}
    assert tiles == {128, SK_TM}                       # nt in (128, 256] and above 256
    assert any(cl.get("empty") for _, _, cl in claims)
    assert any(cl.get("tpl") == 4 and cl.get("queued") == 0 for _, _, cl in claims)
    s3 = {c.plan(w).s3 > 0 for c, w, _ in claims}
    assert s3 == {False, True}
    assert {(c.group, w) for c, w, _ in claims if c.group in ("Ea", "Eb")} == \
        {(g, w) for g in ("Ea", "Eb") for w in (8, 16)}
    runs = {(c.runs, c.fix, c.kind) for c in cases if c.runs}
    assert runs == {(r, f, k) for r, f in ((32, None), (33, None), (33, "ident")) for k in ("join", "sort")}
    assert {c.name.split("-")[-1] for c in cases if c.group == "P"} == {"192", "191"}
    assert any(c.plan(16).D2 == 9 and c.layout(16) == "p48" for c in cases if c.group == "Z")


# ---------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _run(libs, oracles, width, cases):
    cases = [c for c in cases if c.expect[width] is not None]
    assert cases
    M.run_cases(libs, oracles, width, cases, check=check_record)


def _at(rows):
    """(width, row) wherever the row's layout exists at that width."""
    return [pytest.param(w, row, id=f"w{w}-{row}") for w in (8, 16) for row in rows
            if w in _widths(row)]


@gpu
def test_no_record_before_a_bucket_pass(libs, width):
    """A fresh workspace has no record, and a sort of nothing (which returns
    before the bucket pass) leaves none."""
    lib = libs[width]
    lib.reset_workspace()
    try:
        assert lib.skew_stats() is None
        lib.dev_sort(lib.empty(0), lib.empty(0))
        assert lib.skew_stats() is None
    finally:
        lib.reset_workspace()


@gpu
@pytest.mark.parametrize("width,row", _at(R_ROWS))
def test_run_length_at_runmax(libs, oracles, width, row):
    """R: 32 copies of every key are fixed in LDS, 33 identical ones pass as
    ordered, 33 differing ones queue every group (join and sort)."""
    _run(libs, oracles, width, group_r(row))


@gpu
@pytest.mark.parametrize("fix", [None, "ident"], ids=["shuffled", "equal"])
@pytest.mark.parametrize("width,row", _at(Z_ROWS))
def test_group_size_classes(libs, oracles, width, row, fix):
    """Z: the hot group at GS_CAP, GS_CAP + 1 on either side, kSkewSmall,
    kSkewSmall + 1 on either side, 5 + 3 work items, and without the hot key in
    R or any tuple in S."""
    _run(libs, oracles, width, group_z(row, fix))


@gpu
def test_group_size_classes_p40(libs, oracles, width):
    """Z at D2 = 9: the 16-byte library's 48-bit words without their group digit."""
    cases = z_p40()
    assert all(c.plan(width).D2 == 9 for c in cases)
    _run(libs, oracles, width, cases)


@gpu
@pytest.mark.parametrize("copies", sorted({c[0] for c in K_CASES}))
@pytest.mark.parametrize("width,row", _at(K_ROWS))
def test_many_keys_in_a_queued_group(libs, oracles, width, row, copies):
    """K: 2048 keys c times each in one group or across two: every bin of the
    cursor scans, every digit's reservations, the slices of k_skew_check."""
    cases = [c for c in group_k(row) if c.name.split("-")[2] == str(copies)]
    for c in cases:
        _, _, cnt = expected(c, width, oracles[width])
        assert cnt >= 2048 * copies * copies
    _run(libs, oracles, width, cases)


@gpu
@pytest.mark.parametrize("width,row", _at(E_ROWS))
def test_inexact_digits_in_a_queued_group(libs, oracles, width, row):
    """E: a queued group under s3 > 0 and under a hint narrower than the data:
    copied unsorted, then the segmented sort and the batched count."""
    _run(libs, oracles, width, group_e(row))


_T = group_t()


@gpu
@pytest.mark.parametrize("width,name", [pytest.param(w, c.name, id=f"w{w}-{c.name}")
                                        for w in (8, 16) for c in _T if c.expect[w] is not None])
def test_bucket_tile_counts(libs, oracles, width, name):
    """T: buckets past 64 * TPL tiles (every group queued, empty ones too),
    past SK_TM (run by run), and TPL 4 with nothing queued."""
    _run(libs, oracles, width, [c for c in _T if c.name == name])


@gpu
@pytest.mark.parametrize("width,row", _at(P_ROWS))
def test_pair_mode_queues_single_slots(libs, oracles, width, row):
    """P: sorts whose every third group (of the first 48 / 45) is one key 3000
    or 20 000 times, an even and an odd number of populated groups."""
    _run(libs, oracles, width, group_p(row))
