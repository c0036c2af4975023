"""Expected values of the as-of join (smj_dev_asof_join), a helper of
test_asof_join_abi.py and test_gpu_asof_join.py, and the table of cases the
GPU test runs.

numpy_asof gives, per S tuple, the position of its partner in the sorted key
column of R (-1: none).  With lb / ub the searchsorted positions of the S key
("left" / "right"), the candidates are B = ub - 1 and F = lb, or B = lb - 1
and F = ub when strict; each is filtered by the tolerance and the group, and
nearest takes the survivor at the smaller distance, B on equal distances.
Distances and shifts are taken on Python integers, so nothing wraps around
(numpy_asof_exact), or, where every |key| is below 2^62 and nothing can wrap,
in int64 over the whole column at once (numpy_asof_fast).
double_loop is the plain definition: a scan of all of R per S tuple.
"""
import numpy as np

from band_ref import max_abs
from test_gpu_band_join import saturate
from test_gpu_parity import rand_tuples

DIRECTIONS = ("backward", "forward", "nearest")
MODES = [(d, s) for d in DIRECTIONS for s in (False, True)]   # the 6 mode combinations


FAST_LIMIT = 1 << 62


def fast_ok(Rk, Sk):
    """No difference of two keys can leave int64: the precondition of
    numpy_asof_fast."""
    return max_abs(np.asarray(Rk), np.asarray(Sk)) < FAST_LIMIT


def numpy_asof(Rk, Sk, direction="backward", strict=False, tolerance=None, group_shift=0):
    """int64 r_idx per S row into the sorted key array Rk, -1 for none:
    numpy_asof_fast where its precondition holds (test_blocks_cases.py pins it
    to the exact path), numpy_asof_exact otherwise."""
    fn = numpy_asof_fast if fast_ok(Rk, Sk) else numpy_asof_exact
    return fn(Rk, Sk, direction, strict, tolerance, group_shift)


def numpy_asof_fast(Rk, Sk, direction="backward", strict=False, tolerance=None, group_shift=0):
    """numpy_asof with the distances taken in int64, for a million S tuples
    at a time; only where max |key| < 2^62, so no difference wraps."""
    assert direction in DIRECTIONS and fast_ok(Rk, Sk)
    Rk, Sk = np.asarray(Rk, np.int64), np.asarray(Sk, np.int64)
    nR, nS = len(Rk), len(Sk)
    none = np.full(nS, -1, np.int64)
    if nR == 0 or nS == 0:
        return none
    lb, ub = np.searchsorted(Rk, Sk, "left"), np.searchsorted(Rk, Sk, "right")
    b = (lb if strict else ub) - 1   # -1: no B
    f = ub if strict else lb         # nR: no F
    # a distance is below 2^63: a larger tolerance is no limit
    tol = None if tolerance is None or tolerance >= 1 << 63 else np.int64(tolerance)

    def side(pos, there):
        r = Rk[np.where(there, pos, 0)]
        dist = np.where(there, np.abs(Sk - r), 0)
        ok = there.copy()
        if tol is not None:
            ok &= dist <= tol
        if group_shift:
            ok &= (r >> group_shift) == (Sk >> group_shift)
        return ok, dist

    okb, db = side(b, b >= 0)
    okf, df = side(f, f < nR)
    if direction == "backward":
        return np.where(okb, b, none)
    if direction == "forward":
        return np.where(okf, f, none)
    return np.where(okb & (~okf | (db <= df)), b, np.where(okf, f, none))


def numpy_asof_exact(Rk, Sk, direction="backward", strict=False, tolerance=None, group_shift=0):
    """numpy_asof with the distances and shifts taken on Python integers."""
    assert direction in DIRECTIONS
    Rk, Sk = np.asarray(Rk, np.int64), np.asarray(Sk, np.int64)
    nR, nS = len(Rk), len(Sk)
    none = np.full(nS, -1, np.int64)
    if nR == 0 or nS == 0:
        return none
    lb, ub = np.searchsorted(Rk, Sk, "left"), np.searchsorted(Rk, Sk, "right")
    b = (lb if strict else ub) - 1   # -1: no B
    f = ub if strict else lb         # nR: no F
    s = [int(k) for k in Sk]

    def side(pos, there):
        """(the candidate counts, its distance) per S row."""
        ok, dist = np.zeros(nS, bool), [0] * nS
        for i in np.flatnonzero(there):
            r = int(Rk[pos[i]])
            dist[i] = abs(s[i] - r)
            ok[i] = (tolerance is None or dist[i] <= tolerance) and \
                (group_shift == 0 or (r >> group_shift) == (s[i] >> group_shift))
        return ok, dist

    okb, db = side(b, b >= 0)
    okf, df = side(f, f < nR)
    if direction == "backward":
        return np.where(okb, b, none)
    if direction == "forward":
        return np.where(okf, f, none)
    take_b = okb & (~okf | np.array([x <= y for x, y in zip(db, df)]))
    return np.where(take_b, b, np.where(okf, f, none))


def double_loop(Rk, Sk, direction="backward", strict=False, tolerance=None, group_shift=0):
    """The plain definition: per S row a scan of all of R."""
    out = []
    for s in Sk:
        s = int(s)
        B = F = None
        for p, r in enumerate(Rk):
            r = int(r)
            if r < s or (r == s and not strict):
                B = p                      # the last such position
            if F is None and (r > s or (r == s and not strict)):
                F = p                      # the first such position
        cand = {}
        for name, p in (("B", B), ("F", F)):
            if p is None:
                continue
            r = int(Rk[p])
            if tolerance is not None and abs(s - r) > tolerance:
                continue
            if group_shift and (r >> group_shift) != (s >> group_shift):
                continue
            cand[name] = (p, abs(s - r))
        if direction == "backward":
            pick = cand.get("B")
        elif direction == "forward":
            pick = cand.get("F")
        elif "B" in cand and "F" in cand:
            pick = cand["B"] if cand["B"][1] <= cand["F"][1] else cand["F"]
        else:
            pick = cand.get("B") or cand.get("F")
        out.append(-1 if pick is None else pick[0])
    return np.array(out, np.int64).reshape(-1)


# ---------------------------------------------------------------------------
# the cases of test_gpu_asof_join.py.  Sizes are the smallest that reach each
# path of the kernels: a tile is 512 S elements, the staged window holds 1024
# R keys.
# ---------------------------------------------------------------------------
TILE, RWIN = 512, 1024


def with_keys(t, keys):
    t["key"] = keys
    return t


def tiny(nr, ns):
    def make(width):
        return rand_tuples(width, nr, 3, 5, 8), rand_tuples(width, ns, 4, 5, 9)
    return make


def case_one_one(width):
    return rand_tuples(width, 1, 3, 7, 8), rand_tuples(width, 1, 4, 7, 8)   # both key 7


def s_edge(ns):
    """A ragged (or exactly full) last S tile against 3000 R keys."""
    def make(width):
        return rand_tuples(width, 3000, 21, 0, 3000), rand_tuples(width, ns, 22, 0, 3000)
    return make


def case_dups(width):
    """Duplicates on both sides, negative keys; S reaches above R's last key."""
    return rand_tuples(width, 3000, 5, -200, 200), rand_tuples(width, 4000, 6, -200, 220)


def one_side(below):
    """Every R key below (above) every S key: the windows clamp at R's ends."""
    def make(width):
        R, S = rand_tuples(width, 700, 31, 100, 1000), rand_tuples(width, 1300, 32, 2000, 3000)
        return (R, S) if below else (S, R)
    return make


def case_wide(width):
    """Windows of several thousand keys: searched in global memory."""
    return rand_tuples(width, 20000, 41, 0, 100000), rand_tuples(width, 1500, 42, 0, 100000)


def case_sparse_R(width):
    return rand_tuples(width, 5, 61, 0, 1 << 20), rand_tuples(width, 3000, 62, 0, 1 << 20)


def case_one_R_many_S(width):
    return rand_tuples(width, 1, 51, 1500, 1501), rand_tuples(width, 3000, 52, 0, 3000)


GROUP_SHIFT = 20
S_GROUPS = (-3, -2, -1, 0, 1, 2, 3)
R_GROUPS = (-3, -1, 0, 1, 3)          # R lacks groups -2 and 2


def case_groups(width):
    """Keys g << 20 | t, some groups negative; about one R tuple per 500 t.
    R's t start at 1 and every S group has a tuple at t = 0, whose B lies in
    the group below."""
    def rel(n, seed, groups, t0):
        rng = np.random.default_rng(seed)
        g = rng.choice(np.array(groups, np.int64), n)
        t = rng.integers(t0, 200_000, n, dtype=np.int64)
        g[:len(groups)], t[:len(groups)] = groups, t0
        return with_keys(rand_tuples(width, n, seed), (g << GROUP_SHIFT) | t)
    return rel(2000, 81, R_GROUPS, 1), rel(3000, 82, S_GROUPS, 0)


def fixed(params):
    return lambda width: params


NO_LIMIT = [(None, 0)]
# name -> (relations of a width, [(tolerance, group_shift)] of a width)
CASES = {
    "empty_R": (tiny(0, 5), fixed(NO_LIMIT)),
    "empty_S": (tiny(5, 0), fixed(NO_LIMIT)),
    "one_one": (case_one_one, fixed(NO_LIMIT)),
    "s511": (s_edge(511), fixed(NO_LIMIT)),
    "s512": (s_edge(512), fixed(NO_LIMIT)),
    "s513": (s_edge(513), fixed(NO_LIMIT)),
    "s1025": (s_edge(1025), fixed(NO_LIMIT)),
    "dups": (case_dups, fixed(NO_LIMIT)),
    "all_below": (one_side(True), fixed(NO_LIMIT)),
    "all_above": (one_side(False), fixed(NO_LIMIT)),
    "wide": (case_wide, fixed(NO_LIMIT)),
    "sparse_R": (case_sparse_R, fixed([(0, 0), (1000, 0), (None, 0)])),
    "one_R_many_S": (case_one_R_many_S, fixed(NO_LIMIT)),
    "groups": (case_groups, fixed([(None, GROUP_SHIFT), (500, GROUP_SHIFT)])),
    "ends": (saturate("both"), fixed([(None, 0), ((1 << 63) + 7, 0), (40, 0), (0, 0)])),
}
# (case, tolerance, group_shift) whose description promises matched and
# unmatched rows, in each of the 6 mode combinations
MIXED = [("sparse_R", 1000, 0), ("groups", None, GROUP_SHIFT), ("groups", 500, GROUP_SHIFT)]
_inputs, _expected = {}, {}


def inputs(orc, width, name):
    """Sorted inputs of a case, computed once."""
    if (width, name) not in _inputs:
        R, S = CASES[name][0](width)
        R, S = orc.sort(R), orc.sort(S)
        for a in (R, S):
            a.setflags(write=False)
        _inputs[width, name] = (R, S)
    return _inputs[width, name]


def expected(orc, width, name, direction, strict, tolerance, group_shift):
    """r_idx of a case in a mode, computed once."""
    key = (width, name, direction, strict, tolerance, group_shift)
    if key not in _expected:
        R, S = inputs(orc, width, name)
        idx = numpy_asof(R["key"], S["key"], direction, strict, tolerance, group_shift)
        idx.setflags(write=False)
        _expected[key] = idx
    return _expected[key]


def tile_windows(Rk, Sk):
    """The number of R keys in the window of every S tile: from one below the
    lower bound of the tile's first key to one past the upper bound of its
    last, clamped to R."""
    out = []
    for tb in range(0, len(Sk), TILE):
        lo = max(int(np.searchsorted(Rk, Sk[tb], "left")) - 1, 0)
        hi = min(int(np.searchsorted(Rk, Sk[min(tb + TILE, len(Sk)) - 1], "right")) + 1, len(Rk))
        out.append(hi - lo)
    return out
