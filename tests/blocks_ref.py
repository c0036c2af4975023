"""The cases of test_gpu_join_blocks.py: sorted relations whose S spans three
blocks of the tile scan, and their expected values.  No device use
(test_blocks_cases.py checks on the CPU that every case holds what its
description promises).

The join-output operators cut S into tiles and run bounds kernel, count pass,
scan, write pass (materialize.hip's header).  The geometry, restated once:
"""
import numpy as np

import asof_ref
import band_ref
import outer_ref
from test_gpu_join_index import numpy_pairs, numpy_semi_mask
from test_gpu_parity import rand_tuples

TILE = 512     # S elements per tile: MT_TILE, csrc/mat_common.hpp:19
RWIN = 1024    # R keys staged in LDS: MT_RWIN, csrc/mat_common.hpp:20
PIECE = 8192   # output rows per work item: kMatPiece, csrc/mat_common.hpp:21
SCAN = 1024    # tiles per scan block: MS_BLOCK, csrc/materialize.hip:159 (and the count
#                forms' TT_BLOCK, materialize.hip:260)
BOUNDS = 256   # tiles per workgroup of a bounds kernel: csrc/materialize.hip:61 (bandjoin.hip:65,
#                asofjoin.hip:55, outerjoin.hip:82), launched by smj_internal.hpp:495

# 2050 tiles in three scan blocks, the last of two tiles, the last tile of one
# element; nine workgroups of a bounds kernel.  Three blocks, not two: the
# third block's base is a sum of two parts
NS3 = 2 * SCAN * TILE + TILE + 1
CUT = SCAN * TILE          # the first S position of scan block 1 (tile 1024)
MAX_ROWS = 6_000_000       # no operator on any case returns more

BANDS = [(0, 0), (-1, 1)]
TOLERANCES = [None, 2]


def with_keys(t, keys):
    t["key"] = keys
    return t


def ntiles(n):
    return (n + TILE - 1) // TILE


def items(count):
    """work items of a tile with `count` output rows"""
    return (count + PIECE - 1) // PIECE


# ---------------------------------------------------------------------------
# the cases: width -> unsorted (R, S).  The keys do not depend on the width.
# ---------------------------------------------------------------------------
R_KEYS, S_KEYS = 800_000, 1_060_000
# no R tuple has a key in HOLE.  Sorted S is uniform over 1..S_KEYS, position p
# holds about key p * S_KEYS / NS3, so the S tuples with a key in HOLE lie at
# about tiles 990..1059: tiles 1004..1044 hold such keys only
HOLE = (512_000, 548_000)
EMPTY_TILES = (1004, 1044)


def case_keyjoin3(width):
    """R: the keys 1..800 000 outside HOLE, each once; S uniform over
    1..1 060 000, so about a quarter of S has no partner.  Every tile is a
    bitmap tile and tiles 1004..1044, on both sides of the block boundary at
    tile 1024, have count 0."""
    keys = np.arange(1, R_KEYS + 1)
    keys = keys[(keys < HOLE[0]) | (keys > HOLE[1])]
    R = with_keys(rand_tuples(width, len(keys), 301), np.random.default_rng(303).permutation(keys))
    return R, rand_tuples(width, NS3, 302, 1, S_KEYS + 1)


def case_dups3(width):
    """300 000 R tuples and S, keys uniform in 1..260 000: multi tiles
    throughout, S runs straddling most tile edges, about 1.2 M pairs."""
    return rand_tuples(width, 300_000, 311, 1, 260_001), rand_tuples(width, NS3, 312, 1, 260_001)


HOT_S_RUN = 1100 * TILE              # S tuples of the hot key
HOT_S_BEGIN = 500 * TILE + TILE // 2  # its first sorted position: the middle of tile 500
HOT_S_KEY = 3 * (HOT_S_BEGIN + 1)


def case_hot_S(width):
    """One key fills 1100 tiles' worth of S, from the middle of tile 500 to
    the middle of tile 1600: across the block boundary and four workgroups of
    a bounds kernel.  R holds it three times.  The other S keys are multiples
    of 3, each once; R has three quarters of them once, and every fifth of
    them plus 1, which S lacks."""
    below, above = HOT_S_BEGIN, NS3 - HOT_S_BEGIN - HOT_S_RUN
    other = np.concatenate([3 * np.arange(1, below + 1), HOT_S_KEY + 3 * np.arange(1, above + 1)])
    i = np.arange(len(other))
    rk = np.concatenate([other[i % 4 != 0], other[i % 5 == 0] + 1, [HOT_S_KEY] * 3])
    sk = np.concatenate([other, np.full(HOT_S_RUN, HOT_S_KEY)])
    rng = np.random.default_rng(323)
    return (with_keys(rand_tuples(width, len(rk), 321), rng.permutation(rk)),
            with_keys(rand_tuples(width, NS3, 322), rng.permutation(sk)))


HOT_R_RUN = 40_000   # R tuples of the hot key
HOT_R_HALF = 30      # S tuples of it on either side of the block boundary


def hot_R_key(slot):
    """keys 1, 2, 4, 5, 7, 8, ...: every key has one neighbour at distance 1"""
    return 1 + slot + slot // 2


HOT_R_KEY = hot_R_key(CUT - HOT_R_HALF)


def case_hot_R(width):
    """R holds one key 40 000 times (no tile's window with it is staged); S
    holds it 60 times, at the sorted positions CUT - 30 .. CUT + 30: 30 in
    tile 1023, the last of scan block 0, and 30 in tile 1024.  Every other S
    key occurs once on each side.  Tiles 1023 and 1024 carry 1.2 M pairs each,
    147 work items, between tiles of one work item."""
    keys = hot_R_key(np.arange(NS3 - 2 * HOT_R_HALF + 1))
    hot = keys == HOT_R_KEY
    rk = np.concatenate([keys[~hot], np.full(HOT_R_RUN, HOT_R_KEY)])
    sk = np.concatenate([keys[~hot], np.full(2 * HOT_R_HALF, HOT_R_KEY)])
    rng = np.random.default_rng(333)
    return (with_keys(rand_tuples(width, len(rk), 331), rng.permutation(rk)),
            with_keys(rand_tuples(width, NS3, 332), rng.permutation(sk)))


GAP_RUNS = {"front": 9_000, "boundary": 100_000, "tail": 20_000}


def case_gaps(width):
    """keyjoin3 with every key doubled, and three R-only runs of one (odd) key
    each: 9 000 tuples in front of every S key; 100 000 strictly between the S
    keys at the sorted positions CUT - 1 and CUT, a gap of 13 work items owned
    by the first element of tile 1024; 20 000 above every S key, the tail,
    owned by the one-element last tile.  (Where the two S keys around CUT are
    equal, the tuples of that key from CUT on get the next key.)"""
    R, S = case_keyjoin3(width)
    sk = np.sort(S["key"])
    k = sk[CUT - 1]
    move = int(np.searchsorted(sk, k, "right")) - CUT
    S["key"][np.flatnonzero(S["key"] == k)[:move]] = k + 1
    R["key"] *= 2
    S["key"] *= 2
    extra = np.concatenate([np.full(GAP_RUNS["front"], -7),
                            np.full(GAP_RUNS["boundary"], 2 * k + 1),
                            np.full(GAP_RUNS["tail"], 2 * S_KEYS + 11)])
    Rx = with_keys(rand_tuples(width, len(extra), 341), extra)
    R = np.concatenate([R, Rx])
    return R[np.random.default_rng(343).permutation(len(R))], S


def case_only_S(width):
    """R empty, S of NS3 tuples (k_outer_side beyond its first workgroups)"""
    return rand_tuples(width, 0, 351), case_dups3(width)[1]


def case_only_R(width):
    R, S = case_only_S(width)
    return S, R


CASES = {"keyjoin3": case_keyjoin3, "dups3": case_dups3, "hot_S": case_hot_S,
         "hot_R": case_hot_R, "gaps": case_gaps, "only_S": case_only_S, "only_R": case_only_R}
JOIN_CASES = ["keyjoin3", "dups3", "hot_S", "hot_R"]     # pairs, materialize, semi, anti
RANGE_CASES = ["keyjoin3", "dups3", "hot_R"]             # band, as-of
OUTER_CASES = JOIN_CASES + ["gaps"]
SIDE_CASES = ["only_S", "only_R"]

_inputs, _keys, _expected = {}, {}, {}


def inputs(orc, width, name):
    """The sorted, read-only inputs of a case, made once per width.  Both
    widths of a case have the same sorted keys, so that the expected positions
    below, which follow from the keys alone, are computed once for both."""
    if (width, name) not in _inputs:
        R, S = CASES[name](width)
        R, S = (orc.sort(t) if len(t) else t for t in (R, S))
        for a in (R, S):
            a.setflags(write=False)
        keys = _keys.setdefault(name, (R["key"].astype(np.int64), S["key"].astype(np.int64)))
        assert np.array_equal(keys[0], R["key"]) and np.array_equal(keys[1], S["key"]), name
        _inputs[width, name] = (R, S)
    return _inputs[width, name]


def cached(key, make):
    """Expected positions of (case, operator, arguments), computed once: held
    as read-only int32 (no position or key of a case needs more)."""
    if key not in _expected:
        out = make()
        out = tuple(small(a) for a in out) if isinstance(out, tuple) else small(out)
        _expected[key] = out
    return _expected[key]


def small(a):
    if a.dtype != bool:
        assert len(a) == 0 or (-(1 << 31) <= a.min() and a.max() < 1 << 31)
        a = a.astype(np.int32)
    a.setflags(write=False)
    return a


def pairs(orc, width, name):
    """numpy_pairs: (r_idx, s_idx) per output row"""
    R, S = inputs(orc, width, name)
    return cached((name, "pairs"), lambda: numpy_pairs(R, S))


def semi_mask(orc, width, name, swapped=False):
    """numpy_semi_mask: the S tuples with a partner (swapped: the R tuples)"""
    R, S = inputs(orc, width, name)
    return cached((name, "semi", swapped),
                  lambda: numpy_semi_mask(S, R) if swapped else numpy_semi_mask(R, S))


def band(orc, width, name, lo_hi):
    R, S = inputs(orc, width, name)
    return cached((name, "band", lo_hi), lambda: band_ref.numpy_band(R["key"], S["key"], *lo_hi))


def asof(orc, width, name, direction, strict, tolerance):
    R, S = inputs(orc, width, name)
    return cached((name, "asof", direction, strict, tolerance),
                  lambda: asof_ref.numpy_asof(R["key"], S["key"], direction, strict, tolerance, 0))


def outer(orc, width, name, how):
    """numpy_outer: (r_idx, s_idx, key) per row"""
    R, S = inputs(orc, width, name)
    return cached((name, "outer", how),
                  lambda: outer_ref.numpy_outer(R["key"], S["key"], outer_ref.KEEP[how]))


def first_row_in_tile(s_idx, tile=SCAN):
    """index of the first expected row whose S tuple lies in `tile`"""
    hit = np.flatnonzero(np.asarray(s_idx) // TILE == tile)
    assert len(hit), "no row of that tile"
    return int(hit[0])


def capacities(total, c):
    """The capacity cuts of a call with `total` rows: around one work item,
    around the first row c of tile 1024, and one short of everything."""
    caps = [1, PIECE - 1, PIECE, PIECE + 1, c - 1, c, c + 1, total - 1]
    assert all(0 < x < total for x in caps), (caps, total)
    return caps


# ---------------------------------------------------------------------------
# what the descriptions promise, from the sorted keys and the geometry alone
# ---------------------------------------------------------------------------
def per_tile(values):
    """sums of a per-S-element array over the tiles"""
    return np.add.reduceat(np.asarray(values, np.int64), np.arange(0, len(values), TILE))


def match_counts(Rk, Sk):
    """|R_k| per S element"""
    return np.searchsorted(Rk, Sk, "right") - np.searchsorted(Rk, Sk, "left")


def tile_windows(Rk, Sk):
    """the R keys between the lower bound of every tile's first key and the
    upper bound of its last (k_mat_bounds)"""
    first = Sk[::TILE]
    last = Sk[np.minimum(np.arange(TILE, len(Sk) + TILE, TILE), len(Sk)) - 1]
    return np.searchsorted(Rk, last, "right") - np.searchsorted(Rk, first, "left")


def totals(Rk, Sk, outer_only=False):
    """the number of rows of every operator the GPU module runs on a case"""
    rc = match_counts(Rk, Sk)
    n = int(rc.sum())
    r_only, s_only = int((match_counts(Sk, Rk) == 0).sum()), int((rc == 0).sum())
    out = {"outer_inner": n, "outer_left": n + r_only, "outer_right": n + s_only,
           "outer_full": n + r_only + s_only}
    if not outer_only:
        out.update(pairs=n, semi=len(Sk) - s_only, anti=s_only, asof=len(Sk))
        for lo, hi in BANDS:
            cnt = np.searchsorted(Rk, Sk + hi, "right") - np.searchsorted(Rk, Sk + lo, "left")
            out[f"band_{lo}_{hi}"] = int(cnt.sum())
    return out
