"""Expected values of the window functions (smj_dev_window), a helper of
test_window_abi.py and test_gpu_window.py, and the table of cases the GPU test
runs.

numpy_window gives the seven columns of a relation, one row per tuple.  The
group heads are group_ref.numpy_groups': the positions where key >> shift
differs from the element in front (an arithmetic shift of the int64 key); the
key heads are where the key itself does.  h(i) and p(i), the last group head
and key head at or before i, are running maxima of the head positions.  The
running sum is an int64 cumsum minus its value in front of the head (both wrap
modulo 2^64); running minimum and maximum are np.minimum.accumulate and
np.maximum.accumulate per group.  loop_window is the plain definition on
Python integers, with the sum reduced modulo 2^64 at the end.

The cases are every case of group_ref.CASES and those that reach the key
level (rank, dense_rank), the smallest shapes at which it can go wrong.
"""
import numpy as np

import group_ref as G
from test_gpu_parity import rand_tuples

# the geometry of the kernels (csrc/window.hip, csrc/ga_common.hpp): a
# workgroup of the count and write passes handles T elements, one of the carry
# step B tiles
T = 1024
B = 1024
COLUMNS = ("group", "row", "rank", "dense_rank", "sum", "min", "max")


def heads(t, shift=0):
    """(group heads, key heads) of the structured array t, as bool arrays."""
    n = len(t)
    key = t["key"].astype(np.int64)
    g = key >> shift
    head, khead = np.ones(n, bool), np.ones(n, bool)
    head[1:] = g[1:] != g[:-1]
    khead[1:] = key[1:] != key[:-1]
    return head, khead


def numpy_window(t, shift=0):
    """{column: array} of the structured array t, one row per tuple."""
    n = len(t)
    pdt = t["payload"].dtype
    z = np.zeros(n, np.int64)
    if n == 0:
        return {"group": z, "row": z, "rank": z, "dense_rank": z, "sum": z,
                "min": z.astype(pdt), "max": z.astype(pdt)}
    head, khead = heads(t, shift)
    idx = np.arange(n, dtype=np.int64)
    h = np.maximum.accumulate(np.where(head, idx, 0))
    p = np.maximum.accumulate(np.where(khead, idx, 0))
    only = np.cumsum(khead & ~head).astype(np.int64)   # key heads that are no group heads
    pay = t["payload"].astype(np.int64)
    with np.errstate(over="ignore"):
        cs = np.cumsum(pay)
        total = cs - (cs[h] - pay[h])
    mn, mx = np.empty(n, pdt), np.empty(n, pdt)
    start = np.flatnonzero(head)
    for a, b in zip(start, np.append(start[1:], n)):
        mn[a:b] = np.minimum.accumulate(t["payload"][a:b])
        mx[a:b] = np.maximum.accumulate(t["payload"][a:b])
    return {"group": np.cumsum(head).astype(np.int64) - 1, "row": idx - h, "rank": p - h,
            "dense_rank": only - only[h], "sum": total, "min": mn, "max": mx}


def loop_window(t, shift=0):
    """The plain definition: one pass on Python integers."""
    rows = []
    group, h, p, dense, total, mn, mx = -1, 0, 0, 0, 0, 0, 0
    for i in range(len(t)):
        k, v = int(t["key"][i]), int(t["payload"][i])
        if i == 0 or (k >> shift) != (int(t["key"][i - 1]) >> shift):
            group, h, p, dense, total, mn, mx = group + 1, i, i, 0, 0, v, v
        elif k != int(t["key"][i - 1]):
            p, dense = i, dense + 1
        total, mn, mx = total + v, min(mn, v), max(mx, v)
        s = total % (1 << 64)
        rows.append((group, i - h, p - h, dense, s - (1 << 64) if s >= 1 << 63 else s, mn, mx))
    pdt = t["payload"].dtype
    dts = (np.int64,) * 5 + (pdt, pdt)
    return {c: np.array([r[j] for r in rows], dts[j]).reshape(-1) for j, c in enumerate(COLUMNS)}


# ---------------------------------------------------------------------------
# the cases of test_gpu_window.py: name -> (relation of a width, shift)
# ---------------------------------------------------------------------------
def keyed_runs(width, keys, lengths, seed):
    """Runs of the given keys and lengths under random payloads."""
    t = rand_tuples(width, int(np.sum(lengths)), seed)
    t["key"] = np.repeat(np.array(keys, np.int64), lengths)
    return t


def case_peers_cross_tiles(width):
    """Groups of 2^8 keys.  The second group starts at element 10; its key
    0x101 runs from the middle of tile 0 to the middle of tile 2: for the
    elements of tile 1, p(i) and h(i) both lie in front of the tile."""
    first = T // 2 - 7
    return keyed_runs(width, [5, 0x100, 0x101, 0x102, 0x200],
                      [10, first - 10, 2 * T + T // 2 - first, 50, 30], 81), 8


def case_key_head_at_tile_edges(width):
    """A key head that is no group head at element T - 1, another at T, and a
    group head at 2 T exactly."""
    return keyed_runs(width, [0x100, 0x101, 0x102, 0x200, 0x201], [T - 1, 1, T, 37, 5], 82), 8


FAR = (B + 2) * T + 3


def case_dense_far(width):
    """One group of 2^20 keys over (B + 2) T + 3 tuples in key runs of about
    3: dense_rank reaches about n / 3 through both levels of the carry step."""
    return G.by_key(rand_tuples(width, FAR, 83, 0, FAR // 3)), 20


def case_dense_resets(width):
    """Such a far group ends in the middle of a tile; behind it short groups
    of three distinct keys each."""
    far = (B + 1) * T + T // 2 - 5
    a = G.by_key(rand_tuples(width, far, 84, 0, far // 3))
    keys = [(g << 20) + d for g in range(1, 41) for d in (3, 4, 900)]
    b = keyed_runs(width, keys, [2, 1, 3] * 40, 85)
    return np.concatenate([a, b]), 20


def case_shift0_ranks(width):
    """Repeated keys without a group shift: every key run is a group."""
    return G.by_key(rand_tuples(width, 2 * T + 9, 86, -300, 300)), 0


CASES = dict(G.CASES)
CASES.update({
    "peers_cross_tiles": case_peers_cross_tiles,
    "key_head_at_tile_edges": case_key_head_at_tile_edges,
    "dense_far": case_dense_far,
    "dense_resets": case_dense_resets,
    "shift0_ranks": case_shift0_ranks,
})
NEW = [name for name in CASES if name not in G.CASES]
_inputs, _expected = {}, {}


def inputs(width, name):
    """(relation, shift) of a case, computed once and read-only."""
    if name in G.CASES:
        return G.inputs(width, name)
    if (width, name) not in _inputs:
        t, shift = CASES[name](width)
        t.setflags(write=False)
        _inputs[width, name] = (t, shift)
    return _inputs[width, name]


def expected(width, name):
    """The columns of a case, computed once and read-only."""
    if (width, name) not in _expected:
        cols = numpy_window(*inputs(width, name))
        for c in cols.values():
            c.setflags(write=False)
        _expected[width, name] = cols
    return _expected[width, name]
