"""Expected values of the band join (smj_dev_band_join), a helper of
test_band_join_abi.py and test_gpu_band_join.py.

numpy_band builds the pairs with s.key + lo <= r.key <= s.key + hi from the
sorted key columns: per S tuple the range R[lb, ub) with lb = the first key
>= s.key + lo and ub = the first key > s.key + hi.  The sums are taken as
Python integers, so nothing wraps around, and clipped to int64 for the
searches; an S tuple whose unclipped band lies outside int64 has no partner
(numpy_band_exact).  Where max |key| + max(|lo|, |hi|) < 2^62 no sum can leave
int64 and numpy_band_fast takes them in int64 over the whole column at once.
The output is S-major: S tuples in sorted order, each with its R range in
sorted order.
"""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


FAST_LIMIT = 1 << 62


def max_abs(*arrays):
    """The largest |element| of the arrays as a Python integer (0: all empty)."""
    return max([max(abs(int(a.min())), abs(int(a.max()))) for a in arrays if len(a)] or [0])


def fast_ok(Rk, Sk, lo, hi):
    """No key + lo or key + hi can leave int64: the precondition of
    numpy_band_fast."""
    return max_abs(np.asarray(Rk), np.asarray(Sk)) + max(abs(int(lo)), abs(int(hi))) < FAST_LIMIT


def numpy_band(Rk, Sk, lo, hi):
    """(r_idx, s_idx) into the sorted key arrays Rk, Sk per output position:
    numpy_band_fast where its precondition holds (test_blocks_cases.py pins it
    to the exact path), numpy_band_exact otherwise."""
    if len(Rk) and len(Sk) and lo <= hi and fast_ok(Rk, Sk, lo, hi):
        return numpy_band_fast(Rk, Sk, lo, hi)
    return numpy_band_exact(Rk, Sk, lo, hi)


def rows_of(lb, n):
    """S-major (r_idx, s_idx) of the ranges R[lb, lb + n) per S tuple."""
    s_idx = np.repeat(np.arange(len(n)), n)
    pos = np.arange(n.sum()) - (np.cumsum(n) - n)[s_idx]
    return lb[s_idx] + pos, s_idx


def numpy_band_fast(Rk, Sk, lo, hi):
    """numpy_band with the sums taken in int64, for a million S tuples at a
    time; only where max |key| + max(|lo|, |hi|) < 2^62, so no sum wraps."""
    assert fast_ok(Rk, Sk, lo, hi)
    z = np.zeros(0, np.int64)
    if len(Rk) == 0 or len(Sk) == 0 or lo > hi:
        return z, z
    Rk, Sk = np.asarray(Rk, np.int64), np.asarray(Sk, np.int64)
    lb = np.searchsorted(Rk, Sk + np.int64(lo), "left")
    return rows_of(lb, np.searchsorted(Rk, Sk + np.int64(hi), "right") - lb)


def numpy_band_exact(Rk, Sk, lo, hi):
    """numpy_band with the sums taken on Python integers."""
    z = np.zeros(0, np.int64)
    if len(Rk) == 0 or len(Sk) == 0 or lo > hi:
        return z, z
    Rk = np.asarray(Rk, np.int64)
    a = [int(k) + int(lo) for k in Sk]
    b = [int(k) + int(hi) for k in Sk]
    none = np.array([x > I64_MAX or y < I64_MIN for x, y in zip(a, b)])
    a = np.array([min(max(x, I64_MIN), I64_MAX) for x in a], np.int64)
    b = np.array([min(max(y, I64_MIN), I64_MAX) for y in b], np.int64)
    lb = np.searchsorted(Rk, a, "left")
    n = np.searchsorted(Rk, b, "right") - lb
    n[none] = 0
    s_idx = np.repeat(np.arange(len(Sk)), n)
    pos = np.arange(n.sum()) - (np.cumsum(n) - n)[s_idx]
    return lb[s_idx] + pos, s_idx


def double_loop(Rk, Sk, lo, hi):
    """The plain definition, S-major."""
    return [(i, j) for j, s in enumerate(Sk) for i, r in enumerate(Rk)
            if int(s) + lo <= int(r) <= int(s) + hi]
