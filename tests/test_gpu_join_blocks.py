"""The join-output operators past one scan block of S tiles: dev_join_pairs,
dev_materialize, dev_semi_join, dev_band_join (and its count form),
dev_asof_join, dev_outer_join (and its count form) on S of 2 * 1024 * 512 +
513 tuples -- 2050 tiles, three blocks of the tile scan (k_mat_part / pscan /
down), nine workgroups of a bounds kernel, a one-element last tile.

The cases (blocks_ref.CASES; test_blocks_cases.py checks on the CPU that they
hold what they promise) put what the kernels compute per tile on both sides of
the block boundary at tile 1024: whole tiles of count 0, an S run of 1100
tiles, two tiles of 147 work items each between tiles of one, R-only runs
owned by the first tile of a block and by the last tile.  Every comparison is
bit-exact against the numpy constructions of the smaller tests (numpy_pairs,
numpy_semi_mask, band_ref.numpy_band, asof_ref.numpy_asof,
outer_ref.numpy_outer), at both widths; every call writes into columns with
sentinel room behind its capacity, and the inputs are compared unchanged
after it.  The expected positions are computed once per (case, operator
arguments) and shared by the tests and the widths.

Not reached here: the 64-bit division `(off | sc) >> 32` of k_mat_write and
k_outer_write and band_wide() need 2^32 output rows of one key or R tuples of
one window, not a few seconds' worth (test_total_above_2_32 of the smaller
modules counts such a join and checks its first rows).
"""
import numpy as np
import pytest

import blocks_ref as B
import outer_ref as O
from asof_ref import MODES
from blocks_ref import PIECE
from test_gpu_asof_join import check as check_asof, run_asof
from test_gpu_band_join import check_columns, run_band, unchanged
from test_gpu_join_index import SENTINEL, check_pairs, filled, run_pairs
from test_gpu_outer_join import check_rows, dtype_of, run_outer

pytestmark = pytest.mark.gpu

ROOM = 2 * PIECE + 5   # sentinel elements behind a capacity cut


def on_device(lib, orc, width, name):
    R, S = B.inputs(orc, width, name)
    return R, S, lib.to_device(R), lib.to_device(S)


def counter(start):
    import torch
    return torch.full((1,), start, dtype=torch.int64, device="cuda")


# --------------------------------------------------------------- pairs, semi
@pytest.mark.parametrize("name", B.JOIN_CASES)
def test_pairs_and_materialize(libs, oracles, width, name):
    import torch
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, name)
    r_idx, s_idx = B.pairs(orc, width, name)
    total = len(r_idx)
    assert lib.dev_join_pairs(dR, dS) == total  # count only
    got, (r, s, k) = run_pairs(lib, dR, dS, total)
    assert got == total
    check_pairs((r, s, k), R, S, r_idx, s_idx)
    got, (r2, s2) = run_pairs(lib, dR, dS, total, keys=False)
    assert got == total and np.array_equal(r2, r) and np.array_equal(s2, s)
    # the materialised output: the same S payloads and keys
    mat = lib.to_device(filled(S.dtype, total + 5))
    assert lib.dev_materialize(dR, dS) == total
    assert lib.dev_materialize(dR, dS, mat[:total]) == total
    torch.cuda.synchronize()
    mat = lib.to_host(mat)
    assert np.array_equal(mat["payload"][:total], s) and np.array_equal(mat["key"][:total], k)
    assert np.all(mat["key"][total:] == SENTINEL) and np.all(mat["payload"][total:] == SENTINEL)
    unchanged(lib, dR, dS, R, S)


def run_semi(lib, dR, dS, S, cap, anti, room=3):
    import torch
    out = lib.to_device(filled(S.dtype, cap + room))
    total = lib.dev_semi_join(dR, dS, out[:cap], anti=anti)
    torch.cuda.synchronize()
    out = lib.to_host(out)
    assert np.all(out[cap:]["key"] == SENTINEL) and np.all(out[cap:]["payload"] == SENTINEL)
    return total, out[:cap]


@pytest.mark.parametrize("name", B.JOIN_CASES)
def test_semi_and_anti(libs, oracles, width, name):
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, name)
    mask = B.semi_mask(orc, width, name)
    outs = []
    for anti, m in ((False, mask), (True, ~mask)):
        n = int(m.sum())
        assert lib.dev_semi_join(dR, dS, anti=anti) == n  # count only
        got, out = run_semi(lib, dR, dS, S, n, anti)
        assert got == n and np.array_equal(out, S[m]), anti
        outs.append(out)
    # a partition of S
    assert len(outs[0]) + len(outs[1]) == len(S)
    assert np.array_equal(orc.sort(np.concatenate(outs)), S)
    # the same filter on the R side: the arguments swapped, count only
    assert lib.dev_semi_join(dS, dR) == int(B.semi_mask(orc, width, name, swapped=True).sum())
    unchanged(lib, dR, dS, R, S)


# ---------------------------------------------------------------------- band
@pytest.mark.parametrize("band", B.BANDS, ids=["eq", "pm1"])
@pytest.mark.parametrize("name", B.RANGE_CASES)
def test_band(libs, oracles, width, name, band):
    import torch
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, name)
    r_idx, s_idx = B.band(orc, width, name, band)
    total = len(r_idx)
    assert lib.dev_band_join(dR, dS, *band) == total  # count only
    count = counter(5)
    lib.dev_band_join_count(dR, dS, band[0], band[1], count)
    torch.cuda.synchronize()
    assert int(count.item()) == 5 + total
    got, cols = run_band(lib, dR, dS, band, total)
    assert got == total
    check_columns(cols, R, S, r_idx, s_idx)
    unchanged(lib, dR, dS, R, S)


# --------------------------------------------------------------------- as-of
@pytest.mark.parametrize("tol", B.TOLERANCES, ids=["no_limit", "tol2"])
@pytest.mark.parametrize("name", B.RANGE_CASES)
def test_asof(libs, oracles, width, name, tol):
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, name)
    for direction, strict in MODES:
        what = (name, width, direction, strict, tol)
        r_idx = B.asof(orc, width, name, direction, strict, tol)
        cols, added = run_asof(lib, dR, dS, direction, strict, tol, 0)
        check_asof(cols, added, R, r_idx, what)
        # the count form: every column NULL
        _, n = run_asof(lib, dR, dS, direction, strict, tol, 0, (False, False, False))
        assert n == added, what
    unchanged(lib, dR, dS, R, S)


# --------------------------------------------------------------------- outer
def outer_columns(orc, width, name, how):
    R, S = B.inputs(orc, width, name)
    return O.expected_columns(R, S, *B.outer(orc, width, name, how))


@pytest.mark.parametrize("how", O.HOWS)
@pytest.mark.parametrize("name", B.OUTER_CASES + B.SIDE_CASES)
def test_outer(libs, oracles, width, name, how):
    import torch
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, name)
    exp = outer_columns(orc, width, name, how)
    total = len(exp["r_index"])
    if name in B.SIDE_CASES:
        kept = O.KEEP[how] & (O.KEEP_S if name == "only_S" else O.KEEP_R)
        assert total == (B.NS3 if kept else 0)
    assert lib.dev_outer_join(dR, dS, how) == total  # count only
    count = counter(3)
    lib.dev_outer_join_count(dR, dS, how, count)
    got, cols = run_outer(lib, dR, dS, how, total + 2)
    assert got == total and int(count.item()) == 3 + total
    check_rows(cols, exp, total, (name, how))
    if how == "inner" and total:
        # dev_join_pairs row for row
        n, (r, s, k) = run_pairs(lib, dR, dS, total)
        assert n == total
        for c, p in (("r_out", r), ("s_out", s), ("key_out", k)):
            assert np.array_equal(cols[c][:total], p), c
    torch.cuda.synchronize()
    for d, h in ((dR, R), (dS, S)):
        assert len(h) == 0 or np.array_equal(lib.to_host(d), h)


# ------------------------------------------------------------ capacity cuts
def test_capacity_pairs(libs, oracles, width):
    """hot_R: the cuts around one work item, around the first row of tile
    1024 (inside the hot key's pairs) and one row short of everything."""
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, "hot_R")
    r_idx, s_idx = B.pairs(orc, width, "hot_R")
    total = len(r_idx)
    for cap in B.capacities(total, B.first_row_in_tile(s_idx)):
        got, cols = run_pairs(lib, dR, dS, cap, room=ROOM)
        assert got == total, cap
        check_pairs(cols, R, S, r_idx, s_idx)
    unchanged(lib, dR, dS, R, S)


def test_capacity_outer(libs, oracles, width):
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, "hot_R")
    exp = outer_columns(orc, width, "hot_R", "full")
    total = len(exp["r_index"])
    for cap in B.capacities(total, B.first_row_in_tile(exp["s_index"])):
        got, cols = run_outer(lib, dR, dS, "full", cap, room=ROOM)
        assert got == total, cap
        check_rows(cols, exp, cap, ("hot_R", "full", cap))
    unchanged(lib, dR, dS, R, S)


def test_capacity_band(libs, oracles, width):
    orc, lib = oracles[width], libs[width]
    band = (-1, 1)
    R, S, dR, dS = on_device(lib, orc, width, "dups3")
    r_idx, s_idx = B.band(orc, width, "dups3", band)
    total = len(r_idx)
    for cap in B.capacities(total, B.first_row_in_tile(s_idx)):
        got, cols = run_band(lib, dR, dS, band, cap, room=ROOM)
        assert got == total, cap
        check_columns(cols, R, S, r_idx, s_idx)
    unchanged(lib, dR, dS, R, S)


def test_capacity_semi(libs, oracles, width):
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, "keyjoin3")
    kept = np.flatnonzero(B.semi_mask(orc, width, "keyjoin3"))
    total = len(kept)
    # tile 1024 keeps nothing: the first kept row behind the block boundary
    c = int(np.searchsorted(kept, B.CUT))
    assert kept[c] // B.TILE > B.EMPTY_TILES[1]
    for cap in B.capacities(total, c):
        got, out = run_semi(lib, dR, dS, S, cap, False, room=ROOM)
        assert got == total, cap
        assert np.array_equal(out, S[kept[:cap]]), cap
    unchanged(lib, dR, dS, R, S)


# ---------------------------------------------------------- workspace reuse
def test_workspace_reuse(libs, oracles, width):
    """hot_R, the 3-tuple one_one, hot_R again on one workspace: tables of
    2050 tiles, of one tile and of 2050 again."""
    import test_gpu_join_index as J
    orc, lib = oracles[width], libs[width]
    R, S, dR, dS = on_device(lib, orc, width, "hot_R")
    r_idx, s_idx = B.pairs(orc, width, "hot_R")
    exp = outer_columns(orc, width, "hot_R", "full")
    R1, S1, r1, s1 = J.prepared(orc, width, "one_one")
    d1 = lib.to_device(R1), lib.to_device(S1)
    exp1 = O.expected_columns(R1, S1, *O.numpy_outer(R1["key"], S1["key"], O.KEEP["full"]))
    first = None
    for round_ in range(2):
        got, pair_cols = run_pairs(lib, dR, dS, len(r_idx))
        assert got == len(r_idx)
        check_pairs(pair_cols, R, S, r_idx, s_idx)
        got, outer_cols = run_outer(lib, dR, dS, "full", len(exp["r_index"]))
        assert got == len(exp["r_index"])
        check_rows(outer_cols, exp, got, ("hot_R", round_))
        if first is None:
            first = pair_cols, outer_cols
            got, cols = run_pairs(lib, *d1, len(r1))
            assert got == len(r1) == 1
            check_pairs(cols, R1, S1, r1, s1)
            got, cols = run_outer(lib, *d1, "full", 1)
            assert got == 1
            check_rows(cols, exp1, 1, "one_one")
    assert all(np.array_equal(a, b) for a, b in zip(first[0], pair_cols))
    assert all(np.array_equal(first[1][c], outer_cols[c]) for c in O.COLUMNS)
    unchanged(lib, dR, dS, R, S)
