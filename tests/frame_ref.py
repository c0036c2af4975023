"""Expected values of the sliding window frames (smj_dev_window_frame), a helper
of test_window_frame_abi.py and test_gpu_window_frame.py, and the table of
cases the GPU test runs.

numpy_frame gives the seven columns of a relation, one row per tuple.  The
groups are window_ref's: h(i), the last group head at or before i, is a running
maximum of the head positions, and e(i), the last position of i's group, comes
from the next head.  ROWS bounds are i + lo and i + hi with lo / hi clipped to
+-n (no sum can leave int64 then), cut to [h, e].  RANGE bounds are
np.searchsorted per group on the targets key + lo and key + hi, computed on
Python integers and clipped to int64; a band wholly outside int64 is empty.
The sum is a wrapping cumsum difference, minimum and maximum a sparse-table
range query (level k entry j = elements [j, j + 2^k)), of which only the level
in use is kept.  loop_frame is the plain definition on Python integers.

An empty frame is the library's NULL: -1 in start, 0 in every other column.
"""
import numpy as np

import group_ref as G
import window_ref as W
from test_gpu_parity import rand_tuples

# the geometry of the kernels (csrc/frame.hip, csrc/ga_common.hpp): a workgroup
# of the build and write passes handles T elements, the range minimum's inner
# aligned block is BLK, a workgroup of the scan step covers B tiles
T = 1024
BLK = 64
B = 1024
COLUMNS = ("start", "count", "sum", "min", "max", "first", "last")
MIN, MAX = -(1 << 63), (1 << 63) - 1


def group_ends(t, shift):
    """(h, e) per element: the first and last position of its group."""
    n = len(t)
    head, _ = W.heads(t, shift)
    idx = np.arange(n, dtype=np.int64)
    h = np.maximum.accumulate(np.where(head, idx, 0))
    starts = np.flatnonzero(head).astype(np.int64)
    ends = np.append(starts[1:], n) - 1
    return h, ends[np.cumsum(head) - 1], starts, ends


def frame_bounds(t, shift, unit, lo, hi):
    """(a, b, empty) per element; a and b are meaningless where empty."""
    n = len(t)
    lo, hi = int(lo), int(hi)
    idx = np.arange(n, dtype=np.int64)
    h, e, starts, ends = group_ends(t, shift)
    if unit == "rows":
        a = np.maximum(h, idx + max(-n, min(n, lo)))
        b = np.minimum(e, idx + max(-n, min(n, hi)))
        return a, b, a > b
    assert unit == "range", unit
    key = t["key"].astype(np.int64)
    a, b, out = np.empty(n, np.int64), np.empty(n, np.int64), np.zeros(n, bool)
    for s, f in zip(starts, ends):
        k = key[s:f + 1]
        uniq, inv = np.unique(k, return_inverse=True)
        ka = [int(x) + lo for x in uniq]     # Python integers: no wrap-around
        kb = [int(x) + hi for x in uniq]
        outside = np.array([x > MAX or y < MIN for x, y in zip(ka, kb)], bool)
        ta = np.array([max(MIN, min(MAX, x)) for x in ka], np.int64)
        tb = np.array([max(MIN, min(MAX, y)) for y in kb], np.int64)
        a[s:f + 1] = s + np.searchsorted(k, ta, "left")[inv]
        b[s:f + 1] = s + np.searchsorted(k, tb, "right")[inv] - 1
        out[s:f + 1] = outside[inv]
    return a, b, out | (a > b)


def range_extreme(v, a, b, op):
    """op (np.minimum / np.maximum) of v[a[q] .. b[q]] per query q, by a
    sparse table of which one level is alive at a time."""
    res = np.empty(len(a), v.dtype)
    if len(a) == 0:
        return res
    k = np.frexp((b - a + 1).astype(np.float64))[1] - 1    # floor(log2(length))
    level = v.copy()
    for lv in range(int(k.max()) + 1):
        if lv:
            half = 1 << (lv - 1)
            level = op(level[:-half], level[half:])
        q = np.flatnonzero(k == lv)
        if len(q):
            res[q] = op(level[a[q]], level[b[q] - (1 << lv) + 1])
    return res


def numpy_frame(t, shift=0, unit="rows", lo=MIN, hi=0):
    """{column: array} of the structured array t, one row per tuple."""
    n = len(t)
    pdt = t["payload"].dtype
    cols = {c: np.zeros(n, np.int64 if c in ("start", "count", "sum") else pdt)
            for c in COLUMNS}
    if n == 0:
        return cols
    a, b, empty = frame_bounds(t, shift, unit, lo, hi)
    q = np.flatnonzero(~empty)
    a, b = a[q], b[q]
    pay = t["payload"].astype(np.int64)
    with np.errstate(over="ignore"):
        cs = np.cumsum(pay)
        total = cs[b] - cs[a] + pay[a]
    cols["start"][:] = -1
    cols["start"][q] = a
    cols["count"][q] = b - a + 1
    cols["sum"][q] = total
    cols["min"][q] = range_extreme(t["payload"], a, b, np.minimum)
    cols["max"][q] = range_extreme(t["payload"], a, b, np.maximum)
    cols["first"][q] = t["payload"][a]
    cols["last"][q] = t["payload"][b]
    return cols


def loop_frame(t, shift=0, unit="rows", lo=MIN, hi=0):
    """The plain definition: per row, the positions of its group that the
    frame holds, on Python integers."""
    n = len(t)
    key = [int(k) for k in t["key"]]
    pay = [int(p) for p in t["payload"]]
    g = [k >> shift for k in key]
    rows = []
    for i in range(n):
        h = i
        while h > 0 and g[h - 1] == g[i]:
            h -= 1
        e = i
        while e + 1 < n and g[e + 1] == g[i]:
            e += 1
        if unit == "rows":
            js = [j for j in range(h, e + 1) if i + lo <= j <= i + hi]
        else:
            js = [j for j in range(h, e + 1) if key[i] + lo <= key[j] <= key[i] + hi]
        if not js:
            rows.append((-1, 0, 0, 0, 0, 0, 0))
            continue
        assert js == list(range(js[0], js[-1] + 1)), "a frame is contiguous"
        v = [pay[j] for j in js]
        s = sum(v) % (1 << 64)
        rows.append((js[0], len(js), s - (1 << 64) if s >= 1 << 63 else s, min(v), max(v),
                     v[0], v[-1]))
    pdt = t["payload"].dtype
    dts = (np.int64,) * 3 + (pdt,) * 4
    return {c: np.array([r[j] for r in rows], dts[j]).reshape(-1) for j, c in enumerate(COLUMNS)}


# ---------------------------------------------------------------------------
# the cases of test_gpu_window_frame.py: name -> f(width) = (relation, shift,
# unit, lo, hi)
# ---------------------------------------------------------------------------
def on(name, unit, lo, hi, shift=None):
    """A frame on a case of window_ref (group_ref), at its shift."""
    def make(width):
        t, s = W.inputs(width, name)
        return t, (s if shift is None else shift), unit, lo, hi
    return make


SWEEP_A = (B + 1) * T
SWEEP_SHIFT = 40
SWEEP_FRAME = (-2003, -1990)


def case_range_sweep(width):
    """Part A: (B + 1) T rows of keys j // 1000; part B behind it: T + 7 rows
    of keys 2000 + j.  With RANGE (-2003, -1990) the frame of part B's row j
    is the keys j - 3 .. j + 10 of part A: the lower ends of one write tile's
    rows lie about 1000 positions apart all over part A."""
    t = rand_tuples(width, SWEEP_A + T + 7, 91)
    t["key"][:SWEEP_A] = np.arange(SWEEP_A, dtype=np.int64) // 1000
    t["key"][SWEEP_A:] = 2000 + np.arange(T + 7, dtype=np.int64)
    return (t, SWEEP_SHIFT, "range") + SWEEP_FRAME


EDGE_DOMAINS = ("top", "bottom", "both")
EDGE_FRAMES = ((-30, MAX), (MIN, 30), (MAX, MAX), (MIN, MIN), (-50, 50))
EDGE_SHIFTS = (0, 3, 63)
EDGE_N = 3 * T + 1


def edge_tuples(width, domain):
    """3 T + 1 tuples with keys within 40 of the ends of the key type
    (test_group_aggregate_abi.DOMAINS at int64; the int32 counterparts for
    the 8-byte library), ordered by key."""
    lo, hi = G.limits(width)
    rng = np.random.default_rng(17 + EDGE_DOMAINS.index(domain))
    t = rand_tuples(width, EDGE_N, 92 + EDGE_DOMAINS.index(domain))
    off = rng.integers(0, 40, EDGE_N, dtype=np.int64, endpoint=True)
    top = {"top": np.ones(EDGE_N, bool), "bottom": np.zeros(EDGE_N, bool),
           "both": rng.integers(0, 2, EDGE_N) == 1}[domain]
    t["key"] = np.where(top, hi - off, lo + off)
    return G.by_key(t)


def edge_case(domain, shift, lo, hi):
    def make(width):
        if (width, domain) not in _edge:
            t = edge_tuples(width, domain)
            t.setflags(write=False)
            _edge[width, domain] = t
        return _edge[width, domain], shift, "range", lo, hi
    return make


def fname(lo, hi):
    word = {MIN: "min", MAX: "max"}
    return "_".join(word.get(v, str(v).replace("-", "m")) for v in (lo, hi))


_edge = {}
CASES = {}
for _name in G.CASES:
    CASES[f"rows_m2_1/{_name}"] = on(_name, "rows", -2, 1)
ENDS = [(-(BLK - 2), 0), (-(BLK - 1), 0), (-BLK, 0), (-(T - 2), 0), (-(T - 1), 0), (-T, 0),
        (-5, -2), (-70, 3), (-T - 1, T + 1), (-(3 * T + 7), 2 * T + 1), (2, 5), (-7, -3),
        (2, 1), (MAX, MAX), (MIN, MIN)]
ALL_EMPTY = [(2, 1), (MAX, MAX), (MIN, MIN)]
for _lo, _hi in ENDS:
    CASES[f"ends_{fname(_lo, _hi)}/one_key_short"] = on("one_key_short", "rows", _lo, _hi)
CASES["lag1/key_head_at_tile_edges"] = on("key_head_at_tile_edges", "rows", -1, -1)
CASES["lead1/key_head_at_tile_edges"] = on("key_head_at_tile_edges", "rows", 1, 1)
CASES["lag_other_tile/one_key_short"] = on("one_key_short", "rows", -(T + 5), -(T + 5))
FAR_FRAMES = [(MIN, 0), (MIN, MAX), (-(B + 1) * T, 0), (-(B + 1) * T, -(B + 1) * T)]
for _name in ("one_key_long", "dense_resets"):
    for _lo, _hi in FAR_FRAMES:
        CASES[f"far_{fname(_lo, _hi)}/{_name}"] = on(_name, "rows", _lo, _hi)
RANGE_FRAMES = [(MIN, 0), (0, 0), (-5, 5), (3, 7), (-7, -3), (2, 1)]
for _name in ("peers_cross_tiles", "dense_far"):
    for _lo, _hi in RANGE_FRAMES:
        CASES[f"range_{fname(_lo, _hi)}/{_name}"] = on(_name, "range", _lo, _hi)
CASES["range_m300_300/shift0_ranks"] = on("shift0_ranks", "range", -300, 300, 0)
CASES["range_m5_5/shift63"] = on("shift63", "range", -5, 5)
CASES["range_sweep"] = case_range_sweep
for _d in EDGE_DOMAINS:
    for _s in EDGE_SHIFTS:
        for _lo, _hi in EDGE_FRAMES:
            CASES[f"edge_{_d}_s{_s}_{fname(_lo, _hi)}"] = edge_case(_d, _s, _lo, _hi)
_inputs, _expected = {}, {}


def inputs(width, name):
    """(relation, shift, unit, lo, hi) of a case, computed once and read-only."""
    if (width, name) not in _inputs:
        case = CASES[name](width)
        if case[0].flags.writeable:
            case[0].setflags(write=False)
        _inputs[width, name] = case
    return _inputs[width, name]


def expected(width, name):
    """The columns of a case, read-only; computed once, except for the cases
    past 64 tiles, which one test each runs (seven columns of a million rows
    per case are not worth keeping)."""
    if (width, name) in _expected:
        return _expected[width, name]
    case = inputs(width, name)
    cols = numpy_frame(*case)
    for c in cols.values():
        c.setflags(write=False)
    if len(case[0]) <= 64 * T:
        _expected[width, name] = cols
    return cols
