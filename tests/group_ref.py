"""Expected values of the grouped aggregation (smj_dev_group_aggregate), a
helper of test_group_aggregate_abi.py and test_gpu_group_aggregate.py, and the
table of cases the GPU test runs.

numpy_groups gives the six columns of a relation: the heads are the positions
where key >> shift differs from the element in front (an arithmetic shift of
the int64 key), the sums come from np.add.reduceat over int64 (which wraps
modulo 2^64), minimum and maximum from np.minimum.reduceat and
np.maximum.reduceat.  loop_groups is the plain definition on Python integers,
with the sum reduced modulo 2^64 at the end.

The inputs are ordered by key only (a stable argsort of the keys under random
payloads), so the payloads of a run come in no order.
"""
import numpy as np

from test_gpu_parity import rand_tuples

# the geometry of the kernels (csrc/groupagg.hip): a workgroup of the count
# and write passes handles T elements, one of the carry step B tiles
T = 1024
B = 1024
COLUMNS = ("key", "start", "count", "sum", "min", "max")


def numpy_groups(t, shift=0):
    """{column: array} of the structured array t, one row per group."""
    n = len(t)
    pdt = t["payload"].dtype
    if n == 0:
        z = np.zeros(0, np.int64)
        return {"key": z.astype(t["key"].dtype), "start": z, "count": z, "sum": z,
                "min": z.astype(pdt), "max": z.astype(pdt)}
    g = t["key"].astype(np.int64) >> shift
    head = np.ones(n, bool)
    head[1:] = g[1:] != g[:-1]
    start = np.flatnonzero(head).astype(np.int64)
    count = np.diff(np.append(start, n)).astype(np.int64)
    with np.errstate(over="ignore"):
        total = np.add.reduceat(t["payload"].astype(np.int64), start)
    return {"key": t["key"][start], "start": start, "count": count, "sum": total,
            "min": np.minimum.reduceat(t["payload"], start),
            "max": np.maximum.reduceat(t["payload"], start)}


def loop_groups(t, shift=0):
    """The plain definition: one pass on Python integers."""
    rows = []
    for i in range(len(t)):
        k, p = int(t["key"][i]), int(t["payload"][i])
        if rows and (k >> shift) == rows[-1]["g"]:
            r = rows[-1]
            r["count"] += 1
            r["sum"] += p
            r["min"], r["max"] = min(r["min"], p), max(r["max"], p)
        else:
            rows.append({"g": k >> shift, "key": k, "start": i, "count": 1, "sum": p,
                         "min": p, "max": p})
    for r in rows:
        s = r["sum"] % (1 << 64)
        r["sum"] = s - (1 << 64) if s >= 1 << 63 else s
    pdt = t["payload"].dtype
    dts = {"key": t["key"].dtype, "start": np.int64, "count": np.int64, "sum": np.int64,
           "min": pdt, "max": pdt}
    return {c: np.array([r[c] for r in rows], dts[c]).reshape(-1) for c in COLUMNS}


# ---------------------------------------------------------------------------
# the cases of test_gpu_group_aggregate.py: name -> (relation of a width, shift)
# ---------------------------------------------------------------------------
def limits(width):
    """(smallest, largest) value of the key and payload type."""
    bits = 31 if width == 8 else 63
    return -(1 << bits), (1 << bits) - 1


def by_key(t):
    """t ordered by key only: the payloads of a run stay in random order."""
    return t[np.argsort(t["key"], kind="stable")]


def from_runs(width, lengths, seed, first_key=-3, step=1):
    """Runs of the given lengths, keys first_key, first_key + step, ..."""
    n = int(np.sum(lengths))
    t = rand_tuples(width, n, seed)
    t["key"] = np.repeat(first_key + step * np.arange(len(lengths), dtype=np.int64), lengths)
    return t


def short_runs(n):
    """Keys from a domain about n / 3 wide: runs of about 3."""
    def make(width):
        return by_key(rand_tuples(width, n, 100 + n % 97, -(n // 6) - 1, n // 6 + 1)), 0
    return make


def case_all_distinct(width):
    t = rand_tuples(width, 2 * T + 5, 7)
    t["key"] = np.arange(len(t), dtype=np.int64) * 3 - 1000
    return t, 0


def one_key(n):
    """One group; its smallest and largest payload lie in middle tiles."""
    def make(width):
        t = rand_tuples(width, n, 11)
        t["key"] = 42
        for pick, pos in ((np.argmin, T + T // 2), (np.argmax, 3 * T + 5)):
            i = int(pick(t["payload"]))
            t["payload"][[i, pos]] = t["payload"][[pos, i]]
        return t, 0
    return make


def case_end_at_tile(width):
    """A run ends exactly at element T - 1 and the next starts at T."""
    return from_runs(width, [T - 7, 7, 9, 2 * T - 9 - 3, 3], 21), 0


def case_head_last_of_tile(width):
    """A run whose head is element T - 1."""
    return from_runs(width, [T - 1, 5, T - 4 - 1, 1 + T // 2], 22), 0


def case_mid0_to_mid3(width):
    """A run from the middle of tile 0 to the middle of tile 3, then runs of
    length 1."""
    return from_runs(width, [T // 2, 3 * T] + [1] * (T // 2 + 9), 23), 0


def case_extremes(width):
    """Keys at both ends of the key type; payloads at the ends of theirs: the
    largest value repeated (its int64 sum wraps at 16 bytes and leaves int32 at
    8), the smallest repeated, both alternating, and negative ones."""
    lo, hi = limits(width)
    lengths = [5, T + 3, 2, 300, 3, T + 1, 700]
    keys = [lo, lo + 1, lo + 2, -1, hi - 2, hi - 1, hi]
    t = rand_tuples(width, int(np.sum(lengths)), 31)
    t["key"] = np.repeat(np.array(keys, np.int64), lengths)
    s = np.append(0, np.cumsum(lengths))
    t["payload"][s[0]:s[1]] = hi
    t["payload"][s[1]:s[2]] = hi
    t["payload"][s[2]:s[3]] = lo
    t["payload"][s[3]:s[4]] = -(np.abs(t["payload"][s[3]:s[4]].astype(np.int64)) % 1000003) - 1
    t["payload"][s[5]:s[6]] = np.where(np.arange(lengths[5]) % 2 == 0, lo, hi)
    t["payload"][s[6]:s[7]] = lo
    return t, 0


def signed_keys(shift):
    """Negative and non-negative keys under a group shift; at 63 the groups
    are the two signs."""
    def make(width):
        lo, hi = limits(width)
        near = rand_tuples(width, 2 * T + 77, 41, -300, 300)
        far = rand_tuples(width, 40, 42)
        far["key"][:4] = [lo, lo + 1, hi - 1, hi]
        return by_key(np.concatenate([near, far])), shift
    return make


def case_long_groups(width):
    """Groups of 2^12 keys with some 300 tuples each: every group a run over
    distinct keys, its first key not its last."""
    return by_key(rand_tuples(width, 3 * T + 5, 51, -20000, 20000)), 12


def case_run_length(width):
    t = rand_tuples(width, 4, 61)
    t["key"] = [1, 1, 2, 1]
    return t, 0


CASES = {
    "n1": short_runs(1),
    "nTm1": short_runs(T - 1),
    "nT": short_runs(T),
    "nTp1": short_runs(T + 1),
    "n3Tp1": short_runs(3 * T + 1),
    "all_distinct": case_all_distinct,
    "one_key_short": one_key(5 * T + 3),
    "one_key_long": one_key((B + 2) * T + 3),
    "end_at_tile": case_end_at_tile,
    "head_last_of_tile": case_head_last_of_tile,
    "mid0_to_mid3": case_mid0_to_mid3,
    "extremes": case_extremes,
    "shift3": signed_keys(3),
    "shift63": signed_keys(63),
    "long_groups": case_long_groups,
    "run_length": case_run_length,
}
SIZES = {"n1": 1, "nTm1": T - 1, "nT": T, "nTp1": T + 1, "n3Tp1": 3 * T + 1}
_inputs, _expected = {}, {}


def inputs(width, name):
    """(relation, shift) of a case, computed once and read-only."""
    if (width, name) not in _inputs:
        t, shift = CASES[name](width)
        t.setflags(write=False)
        _inputs[width, name] = (t, shift)
    return _inputs[width, name]


def expected(width, name):
    """The columns of a case, computed once and read-only."""
    if (width, name) not in _expected:
        cols = numpy_groups(*inputs(width, name))
        for c in cols.values():
            c.setflags(write=False)
        _expected[width, name] = cols
    return _expected[width, name]
