"""Outer join of two sorted relations (smj_dev_outer_join): the expected-value
construction and the case table of test_gpu_outer_join.py.  No device use
(test_outer_join_abi.py checks the construction on the CPU).

numpy_outer builds the rows from the definition in smj.h: over the union of
the keys, ascending, a key on both sides gives its pairs R-major, a key on one
side gives that side's run when the side is kept.  double_loop is the same
definition as plain loops.
"""
import numpy as np

from test_gpu_parity import rand_tuples

KEEP_R, KEEP_S = 1, 2
KEEP = {"inner": 0, "left": KEEP_R, "right": KEEP_S, "full": KEEP_R | KEEP_S}
HOWS = list(KEEP)

# the geometry of the kernels (mat_common.hpp): S elements per tile, R keys
# staged in LDS, rows per work item
TILE, RWIN, PIECE = 512, 1024, 8192


def numpy_outer(Rkeys, Skeys, keep):
    """(r_idx, s_idx, key) per row; -1 for an absent side.  Rkeys, Skeys:
    non-decreasing int64 keys; keep: KEEP_R | KEEP_S bits."""
    Rkeys, Skeys = np.asarray(Rkeys, np.int64), np.asarray(Skeys, np.int64)
    keys = np.union1d(Rkeys, Skeys)
    rlo = np.searchsorted(Rkeys, keys, "left")
    rc = np.searchsorted(Rkeys, keys, "right") - rlo
    slo = np.searchsorted(Skeys, keys, "left")
    sc = np.searchsorted(Skeys, keys, "right") - slo
    per = np.where((rc > 0) & (sc > 0), rc * sc,
                   np.where(sc == 0, rc if keep & KEEP_R else 0, sc if keep & KEEP_S else 0))
    run = np.repeat(np.arange(len(keys)), per)
    total = int(per.sum())
    pos = np.arange(total, dtype=np.int64) - (np.cumsum(per) - per)[run]
    div = np.maximum(sc, 1)[run]
    r = np.where(rc[run] > 0, rlo[run] + pos // div, -1).astype(np.int64)
    s = np.where(sc[run] > 0, slo[run] + pos % div, -1).astype(np.int64)
    return r, s, keys[run].astype(np.int64)


def double_loop(Rkeys, Skeys, keep):
    """The plain definition, row by row."""
    rows = []
    for k in sorted(set(np.asarray(Rkeys).tolist()) | set(np.asarray(Skeys).tolist())):
        ri = [i for i, x in enumerate(Rkeys) if x == k]
        si = [j for j, x in enumerate(Skeys) if x == k]
        if ri and si:
            rows += [(i, j, k) for i in ri for j in si]
        elif ri and keep & KEEP_R:
            rows += [(i, -1, k) for i in ri]
        elif si and keep & KEEP_S:
            rows += [(-1, j, k) for j in si]
    a = np.array(rows, np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def expected_columns(R, S, r_idx, s_idx, key):
    """The five columns of the rows (r_idx, s_idx, key) over sorted R and S:
    an absent side is -1 in its index column and 0 in its payload column."""
    dt = R["payload"].dtype
    rp = np.where(r_idx >= 0, R["payload"][np.maximum(r_idx, 0)] if len(R) else 0, 0).astype(dt)
    sp = np.where(s_idx >= 0, S["payload"][np.maximum(s_idx, 0)] if len(S) else 0, 0).astype(dt)
    return {"r_index": r_idx, "s_index": s_idx, "r_out": rp, "s_out": sp,
            "key_out": key.astype(dt)}


COLUMNS = ("r_index", "s_index", "r_out", "s_out", "key_out")


def with_keys(t, keys):
    t["key"] = keys
    return t


def fixed(width, seed, keys):
    keys = np.asarray(keys, np.int64)
    return with_keys(rand_tuples(width, len(keys), seed), keys)


def case_empty_both(width):
    return rand_tuples(width, 0, 1), rand_tuples(width, 0, 2)


def case_empty_R(width):
    return rand_tuples(width, 0, 3), rand_tuples(width, 5, 4, 5, 9)


def case_empty_S(width):
    return rand_tuples(width, 5, 3, 5, 9), rand_tuples(width, 0, 4)


def case_one_one(width):
    return fixed(width, 3, [7]), fixed(width, 4, [7])


def case_one_lt(width):
    return fixed(width, 3, [6]), fixed(width, 4, [7])


def case_one_gt(width):
    return fixed(width, 3, [8]), fixed(width, 4, [7])


def case_disjoint(width):
    """R the even keys, S the odd keys, 3000 each: no pairs; the full join is
    6000 rows alternating sides."""
    return fixed(width, 5, 2 * np.arange(3000)), fixed(width, 6, 2 * np.arange(3000) + 1)


def case_keyjoin(width):
    """R unique keys 1..3000; S 1300 tuples (a ragged last tile) over keys
    1..4000: R-only and S-only rows sprinkled between matches."""
    rng = np.random.default_rng(21)
    R = with_keys(rand_tuples(width, 3000, 1), rng.permutation(3000) + 1)
    return R, rand_tuples(width, 1300, 2, 1, 4001)


def case_dups(width):
    """Duplicates on both sides, negative keys, S runs that straddle tiles."""
    return rand_tuples(width, 3000, 5, -200, 201), rand_tuples(width, 4000, 6, -200, 221)


def case_hot(width):
    """600 R and 1500 S tuples share key 777 (900 000 pairs, more than 100
    work items); 100 S tuples have key 5000 and 300 R tuples key 6000."""
    R = rand_tuples(width, 2300, 11, 0, 2000)
    S = rand_tuples(width, 3000, 12, 0, 2000)
    R["key"][:600] = 777
    R["key"][2000:] = 6000
    S["key"][:1500] = 777
    S["key"][1500:1600] = 5000
    return R, S


def case_r_gaps(width):
    """A leading, an inner and a trailing R-only run, each longer than a work
    item and than the R window; S is 3 tuples."""
    R = fixed(width, 13, [5] * 9000 + [10] * 2 + [15] * 9000 + [35] * 9000)
    return R, fixed(width, 14, [10, 20, 30])


def case_s_only_tiles(width):
    """S keys 1..3000, each once; R has 4 tuples: whole S tiles without a
    partner, one partner in the first tile, two neighbouring ones in the
    second and an R-only row behind everything."""
    return fixed(width, 15, [100, 611, 612, 5000]), fixed(width, 16, np.arange(1, 3001))


def case_straddle(width):
    """Two S runs that each cross a tile boundary, an R-only run between."""
    R = fixed(width, 17, [7] * 3 + [8] * 2000)
    return R, fixed(width, 18, [7] * 1400 + [9] * 700)


def case_mixed(width):
    """keyjoin and dups (keys shifted by 10000) in one call."""
    Ra, Sa = case_keyjoin(width)
    Rb, Sb = case_dups(width)
    Rb["key"] += 10000
    Sb["key"] += 10000
    return np.concatenate([Ra, Rb]), np.concatenate([Sa, Sb])


CASES = {
    "empty_both": case_empty_both, "empty_R": case_empty_R, "empty_S": case_empty_S,
    "one_one": case_one_one, "one_lt": case_one_lt, "one_gt": case_one_gt,
    "disjoint": case_disjoint, "keyjoin": case_keyjoin, "dups": case_dups, "hot": case_hot,
    "r_gaps": case_r_gaps, "s_only_tiles": case_s_only_tiles, "straddle": case_straddle,
    "mixed": case_mixed,
}
_inputs, _expected = {}, {}


def inputs(orc, width, name):
    """The sorted, read-only inputs of a case, made once."""
    if (width, name) not in _inputs:
        R, S = CASES[name](width)
        R, S = (orc.sort(t) if len(t) else t for t in (R, S))
        for a in (R, S):
            a.setflags(write=False)
        _inputs[width, name] = (R, S)
    return _inputs[width, name]


def expected(orc, width, name, how):
    """(r_idx, s_idx, key) of a case, computed once."""
    if (width, name, how) not in _expected:
        R, S = inputs(orc, width, name)
        exp = numpy_outer(R["key"], S["key"], KEEP[how])
        for a in exp:
            a.setflags(write=False)
        _expected[width, name, how] = exp
    return _expected[width, name, how]
