"""The cases of test_gpu_join_blocks.py on the CPU: every case of
blocks_ref.CASES holds what its description promises, computed from the sorted
keys and the restated geometry alone -- conditions on the inputs, not on the
code under test.  No device call is made.

The vectorised paths of the expected-value constructions
(band_ref.numpy_band_fast, asof_ref.numpy_asof_fast) are pinned to the exact
ones: on every existing case of the band and as-of GPU tests where their
precondition holds, and on a 20 000-tuple sample of each new case."""
import numpy as np
import pytest

import asof_ref as A
import band_ref
import blocks_ref as B
import test_gpu_band_join as band_cases
from blocks_ref import CUT, NS3, PIECE, RWIN, SCAN, TILE


def keys(oracles, width, name):
    R, S = B.inputs(oracles[width], width, name)
    return R["key"].astype(np.int64), S["key"].astype(np.int64)


def test_geometry():
    assert (TILE, RWIN, PIECE, SCAN, B.BOUNDS) == (512, 1024, 8192, 1024, 256)
    assert NS3 == 1_049_089
    nt = B.ntiles(NS3)
    assert nt == 2050 and NS3 - (nt - 1) * TILE == 1       # the last tile: one element
    assert -(-nt // SCAN) == 3 and nt - 2 * SCAN == 2       # three scan blocks, the last of two
    assert -(-nt // B.BOUNDS) == 9


@pytest.mark.parametrize("name", B.JOIN_CASES + ["gaps", "only_S"])
def test_S_spans_three_scan_blocks(oracles, width, name):
    Rk, Sk = keys(oracles, width, name)
    assert len(Sk) == NS3
    assert np.all(np.diff(Sk) >= 0) and np.all(np.diff(Rk) >= 0)


def test_keyjoin3(oracles, width):
    Rk, Sk = keys(oracles, width, "keyjoin3")
    assert len(np.unique(Rk)) == len(Rk) and Rk[0] == 1 and Rk[-1] == B.R_KEYS
    rc = B.match_counts(Rk, Sk)
    assert rc.max() == 1                                   # no multi tile
    assert 0.2 < (rc == 0).mean() < 0.3
    cnt = B.per_tile(rc)
    lo, hi = B.EMPTY_TILES
    assert lo < SCAN < hi and hi - lo >= 40
    assert np.all(cnt[lo:hi + 1] == 0)                     # on both sides of tile 1024
    assert np.all(cnt[:900] > 0) and np.all(cnt[1100:1500] > 0)
    assert np.all(cnt[1600:] == 0)                          # the S keys above R's last
    assert np.all(B.items(cnt) <= 1)


def test_dups3(oracles, width):
    Rk, Sk = keys(oracles, width, "dups3")
    assert len(Rk) == 300_000
    rc = B.match_counts(Rk, Sk)
    multi = np.maximum.reduceat(rc, np.arange(0, NS3, TILE)) > 1
    assert np.all(multi[:-1])                              # the last tile is one element
    assert B.tile_windows(Rk, Sk).max() <= RWIN            # every window is staged
    edges = np.arange(TILE, NS3, TILE)
    assert (Sk[edges - 1] == Sk[edges]).mean() > 0.5       # runs straddle most tile edges
    assert 1_100_000 < rc.sum() < 1_300_000


def test_hot_S(oracles, width):
    Rk, Sk = keys(oracles, width, "hot_S")
    H = B.HOT_S_KEY
    first, last = np.searchsorted(Sk, H, "left"), np.searchsorted(Sk, H, "right")
    assert last - first == 1100 * TILE == 563_200
    assert (first // TILE, first % TILE) == (500, TILE // 2)
    assert ((last - 1) // TILE, last % TILE) == (1600, TILE // 2)
    assert first // TILE < SCAN <= (last - 1) // TILE       # the block boundary inside the run
    assert (last - 1) // TILE // B.BOUNDS - first // TILE // B.BOUNDS + 1 >= 4
    assert np.searchsorted(Rk, H, "right") - np.searchsorted(Rk, H, "left") == 3
    # inside the run the run's start lies up to 1100 tiles back
    assert (last - 1 - first) * 3 > 1_680_000
    other_S, other_R = Sk[Sk != H], Rk[Rk != H]
    assert len(np.unique(other_S)) == len(other_S) and len(np.unique(other_R)) == len(other_R)
    both = np.isin(other_S, other_R).mean()
    assert 0.7 < both < 0.8                                 # some S keys lack a partner
    assert 0.15 < (~np.isin(other_R, other_S)).mean() < 0.3  # and some R keys


def test_hot_R(oracles, width):
    Rk, Sk = keys(oracles, width, "hot_R")
    H = B.HOT_R_KEY
    first, last = np.searchsorted(Sk, H, "left"), np.searchsorted(Sk, H, "right")
    assert (first, last) == (CUT - 30, CUT + 30)            # 30 in tile 1023, 30 in tile 1024
    assert np.searchsorted(Rk, H, "right") - np.searchsorted(Rk, H, "left") == 40_000
    win = B.tile_windows(Rk, Sk)
    assert win[SCAN - 1] > RWIN and win[SCAN] > RWIN        # not staged
    assert win[SCAN - 2] <= RWIN and win[SCAN + 1] <= RWIN
    rc = B.match_counts(Rk, Sk)
    assert np.all(rc[Sk != H] == 1)
    other_S, other_R = Sk[Sk != H], Rk[Rk != H]
    assert len(np.unique(other_S)) == len(other_S) and len(np.unique(other_R)) == len(other_R)
    cnt = B.per_tile(rc)
    assert cnt[SCAN - 1] == cnt[SCAN] == 30 * 40_000 + TILE - 30
    assert B.items(cnt[SCAN - 1]) == B.items(cnt[SCAN]) == 147
    assert B.items(cnt[SCAN - 2]) == B.items(cnt[SCAN + 1]) == 1
    # ibase jumps by 147 on either side of the block boundary
    ibase = np.cumsum(B.items(cnt)) - B.items(cnt)
    assert ibase[SCAN] - ibase[SCAN - 1] == 147 and ibase[SCAN + 1] - ibase[SCAN] == 147
    assert ibase[SCAN - 1] == SCAN - 1


def test_gaps(oracles, width):
    Rk, Sk = keys(oracles, width, "gaps")
    assert Sk[CUT - 1] < Sk[CUT]
    only = np.unique(Rk[Rk % 2 != 0])                      # the odd keys: the three runs
    assert len(only) == 3 and not np.isin(only, Sk).any()
    runs = [int(np.searchsorted(Rk, k, "right") - np.searchsorted(Rk, k, "left")) for k in only]
    assert runs == [B.GAP_RUNS["front"], B.GAP_RUNS["boundary"], B.GAP_RUNS["tail"]]
    # the sorted S position each run precedes
    assert [int(np.searchsorted(Sk, k)) for k in only] == [0, CUT, NS3]
    assert Sk[CUT - 1] < only[1] < Sk[CUT]                 # owned by tile 1024's first element
    assert B.items(runs[1]) == 13 and runs[1] > RWIN
    assert (NS3 - 1) % TILE == 0                            # the tail's owner: a one-element tile
    rc = B.match_counts(Rk, Sk)
    cnt = B.per_tile(rc)
    assert np.all(cnt[B.EMPTY_TILES[0]:B.EMPTY_TILES[1] + 1] == 0) and rc.max() == 1


def test_side_only(oracles, width):
    for name, full, empty in (("only_S", 1, 0), ("only_R", 0, 1)):
        rel = B.inputs(oracles[width], width, name)
        assert len(rel[full]) == NS3 and len(rel[empty]) == 0
        assert -(-NS3 // 256) > 4096                       # workgroups of k_outer_side


@pytest.mark.parametrize("name", B.OUTER_CASES)
def test_totals_within_limit(oracles, width, name):
    Rk, Sk = keys(oracles, width, name)
    t = B.totals(Rk, Sk, outer_only=name == "gaps")
    assert max(t.values()) <= B.MAX_ROWS, t
    # every S key of hot_R has a partner: its anti join is empty
    assert all(v > 0 for k, v in t.items() if (name, k) != ("hot_R", "anti")), t
    if name == "hot_R":
        assert t["anti"] == 0
        # room for the capacity cuts: the first row of tile 1024 lies beyond one work item
        assert t["pairs"] > CUT > PIECE + 1


# ---------------------------------------------------------------------------
# the fast reference paths against the exact ones
# ---------------------------------------------------------------------------
def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(band_cases.CASES))
def test_band_fast_path_existing_cases(oracles, width, name):
    R, S = band_cases.inputs(oracles[width], width, name)
    pinned = 0
    for lo, hi in band_cases.CASES[name][1](width):
        if not band_ref.fast_ok(R["key"], S["key"], lo, hi):
            continue
        pinned += 1
        assert same(band_ref.numpy_band_fast(R["key"], S["key"], lo, hi),
                    band_ref.numpy_band_exact(R["key"], S["key"], lo, hi)), (lo, hi)
    # saturated keys and unbounded bands stay on the exact path
    assert pinned or name.startswith("saturate")


def test_band_fast_path_precondition():
    k = np.array([0, (1 << 62) - 5], np.int64)
    assert band_ref.fast_ok(k, k, -4, 4) and not band_ref.fast_ok(k, k, -5, 5)
    assert not band_ref.fast_ok(np.array([band_ref.I64_MIN]), k, 0, 0)
    with pytest.raises(AssertionError):
        band_ref.numpy_band_fast(k, k, -5, 5)


@pytest.mark.parametrize("name", list(A.CASES))
def test_asof_fast_path_existing_cases(oracles, width, name):
    R, S = A.inputs(oracles[width], width, name)
    if not A.fast_ok(R["key"], S["key"]):
        assert name == "ends" and width == 16
        with pytest.raises(AssertionError):
            A.numpy_asof_fast(R["key"], S["key"])
        return
    for tol, gsh in A.CASES[name][1](width):
        for direction, strict in A.MODES:
            fast = A.numpy_asof_fast(R["key"], S["key"], direction, strict, tol, gsh)
            exact = A.numpy_asof_exact(R["key"], S["key"], direction, strict, tol, gsh)
            assert np.array_equal(fast, exact) and fast.dtype == exact.dtype, \
                (direction, strict, tol, gsh)


def sample(Sk):
    """20 000 sorted S keys of a case: 1 000 around the block boundary and
    19 000 positions drawn from all of S"""
    near = np.arange(CUT - 500, CUT + 500)
    far = np.random.default_rng(7).choice(len(Sk), 19_000, replace=False)
    pos = np.unique(np.concatenate([near, far]))
    rest = np.setdiff1d(np.arange(len(Sk)), pos)[:20_000 - len(pos)]
    return Sk[np.sort(np.concatenate([pos, rest]))]


@pytest.mark.parametrize("name", B.RANGE_CASES)
def test_fast_paths_new_cases(oracles, width, name):
    Rk, Sk = keys(oracles, width, name)
    Sk = sample(Sk)
    assert len(Sk) == 20_000
    for lo, hi in B.BANDS:
        assert band_ref.fast_ok(Rk, Sk, lo, hi)
        assert same(band_ref.numpy_band_fast(Rk, Sk, lo, hi),
                    band_ref.numpy_band_exact(Rk, Sk, lo, hi)), (lo, hi)
    assert A.fast_ok(Rk, Sk)
    for tol in B.TOLERANCES:
        for direction, strict in A.MODES:
            assert np.array_equal(A.numpy_asof_fast(Rk, Sk, direction, strict, tol, 0),
                                  A.numpy_asof_exact(Rk, Sk, direction, strict, tol, 0)), \
                (direction, strict, tol)
