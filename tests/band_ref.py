"""Expected values of the band join (smj_dev_band_join), a helper of
test_band_join_abi.py and test_gpu_band_join.py.

numpy_band builds the pairs with s.key + lo <= r.key <= s.key + hi from the
sorted key columns: per S tuple the range R[lb, ub) with lb = the first key
>= s.key + lo and ub = the first key > s.key + hi.  The sums are taken as
Python integers, so nothing wraps around, and clipped to int64 for the
searches; an S tuple whose unclipped band lies outside int64 has no partner.
The output is S-major: S tuples in sorted order, each with its R range in
sorted order.
"""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def numpy_band(Rk, Sk, lo, hi):
    """(r_idx, s_idx) into the sorted key arrays Rk, Sk per output position."""
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
