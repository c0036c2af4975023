"""The sliding window frames on CPU: both libraries export
smj_dev_window_frame, smj_frame_tile and smj_frame_block, and the binding
carries them up to Library.dev_window_frame / frame_tile / frame_block /
rolling.  No device call is made (tests/test_gpu_window_frame.py runs them; the
two geometry calls are host calls).  The expected-value construction of the
GPU tests (frame_ref.numpy_frame) is checked here against the plain definition
and against window_ref.numpy_window and group_ref.numpy_groups, and the cases
of the GPU test are checked to hold what their descriptions promise:
conditions on the inputs and on the reference, never on the code under test."""
import ctypes
import os

import numpy as np
import pytest

import frame_ref as F
import group_ref as G
import window_ref as W
from test_group_aggregate_abi import DOMAINS, I64_MAX, I64_MIN, domain_tuples

NAMES = ("smj_dev_window_frame", "smj_frame_tile", "smj_frame_block")
MIN, MAX = F.MIN, F.MAX
MATRIX = [(-2, 1), (MIN, 0), (MIN, MAX), (-1, -1), (1, 1), (3, 7), (-7, -3), (2, 1), (0, 0),
          (-5, 5), (MAX, MAX), (MIN, MIN), (-30, MAX)]


@pytest.fixture(scope="module")
def smj_mod():
    import smj
    for w in (8, 16):
        if not os.path.exists(smj.lib_path(w)):
            smj.build()
            break
    return smj


@pytest.mark.parametrize("width", [8, 16])
def test_libraries_export_window_frame(smj_mod, width):
    lib = ctypes.CDLL(smj_mod.lib_path(width))
    for name in NAMES:
        assert hasattr(lib, name), name


def test_names_are_listed(smj_mod):
    for name in NAMES:
        assert name in smj_mod.DEVICE_SYMBOLS
    assert smj_mod.FRAME_UNITS == {"rows": 0, "range": 1}


@pytest.mark.parametrize("width", [8, 16])
def test_binding_has_window_frame(smj_mod, width):
    L = smj_mod.Library(width)
    # (ws, sorted, n, group_shift, unit, lo, hi, start, count, sum, min, max, first, last,
    #  stream)
    f = L.lib.smj_dev_window_frame
    assert f.restype is None
    assert len(f.argtypes) == 15
    assert f.argtypes[2] is ctypes.c_uint64
    assert f.argtypes[3] is ctypes.c_uint32 and f.argtypes[4] is ctypes.c_uint32
    assert f.argtypes[5] is ctypes.c_int64 and f.argtypes[6] is ctypes.c_int64
    assert L.lib.smj_frame_tile.restype is ctypes.c_uint32
    assert L.lib.smj_frame_block.restype is ctypes.c_uint32
    for method in ("dev_window_frame", "frame_tile", "frame_block", "rolling"):
        assert callable(getattr(L, method)), method


@pytest.mark.parametrize("width", [8, 16])
def test_geometry_is_the_kernels(smj_mod, width):
    L = smj_mod.Library(width)
    assert L.frame_tile() == F.T and L.frame_block() == F.BLK
    assert F.T % F.BLK == 0
    assert (F.T, F.B) == (W.T, W.B)


def test_arguments_are_checked(smj_mod):
    L = smj_mod.Library(16)
    assert L._frame("rows", None, None) == (0, MIN, MAX)
    assert L._frame("range", -60, 0) == (1, -60, 0)
    with pytest.raises((ValueError, AssertionError)):
        L._frame("groups", 0, 0)
    with pytest.raises(AssertionError):
        L._frame("rows", MIN - 1, 0)
    with pytest.raises(AssertionError):
        L._group_shift(64)
    # dev_window_frame refuses both before it touches the device
    with pytest.raises((ValueError, AssertionError)):
        L.dev_window_frame(None, 0, "groups")
    with pytest.raises(AssertionError):
        L.dev_window_frame(None, 64)


@pytest.mark.parametrize("domain", list(DOMAINS))
@pytest.mark.parametrize("shift", [0, 3, 63])
@pytest.mark.parametrize("unit", ["rows", "range"])
def test_numpy_construction_against_plain_loop(unit, shift, domain):
    t = domain_tuples(domain, 150, np.random.default_rng(5))
    for lo, hi in MATRIX:
        got, exp = F.numpy_frame(t, shift, unit, lo, hi), F.loop_frame(t, shift, unit, lo, hi)
        for c in F.COLUMNS:
            assert got[c].dtype == exp[c].dtype and np.array_equal(got[c], exp[c]), (lo, hi, c)
    # some frame's sum left int64 on the way (it is kept modulo 2^64)
    a, b, empty = F.frame_bounds(t, shift, unit, MIN, 0)
    true = [sum(int(p) for p in t["payload"][x:y + 1]) for x, y in zip(a, b)]
    assert not empty.any() and any(not I64_MIN <= s <= I64_MAX for s in true)


def test_run_length_form_and_empty():
    t = np.zeros(4, np.dtype([("payload", "<i4"), ("key", "<i4")]))
    t["key"], t["payload"] = [1, 1, 2, 1], [4, -9, 3, 8]
    for f in (F.numpy_frame, F.loop_frame):
        g = f(t, 0, "rows", -1, 0)
        assert g["start"].tolist() == [0, 0, 2, 3] and g["count"].tolist() == [1, 2, 1, 1]
        assert g["sum"].tolist() == [4, -5, 3, 8] and g["first"].tolist() == [4, 4, 3, 8]
        g = f(t, 0, "rows", -1, -1)   # LAG(1)
        assert g["start"].tolist() == [-1, 0, -1, -1] and g["first"].tolist() == [0, 4, 0, 0]
        assert g["count"].tolist() == [0, 1, 0, 0] and g["min"].tolist() == [0, 4, 0, 0]
        assert g["min"].dtype == np.int32 and g["sum"].dtype == np.int64
        assert all(len(v) == 0 for v in f(t[:0]).values())
        assert [v.dtype for v in f(t[:0]).values()] == [np.int64] * 3 + [np.int32] * 4


IDENTITY_CASES = ("n3Tp1", "extremes", "shift3", "shift63", "long_groups", "run_length",
                  "peers_cross_tiles", "key_head_at_tile_edges", "shift0_ranks")


@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_identities_of_the_reference(width, name):
    """What ties the frames to the window functions and to the group table."""
    t, shift = W.inputs(width, name)
    w, g = W.expected(width, name), G.numpy_groups(t, shift)
    n = len(t)
    idx = np.arange(n)
    # ROWS (MIN, 0) is smj_dev_window's frame
    f = F.numpy_frame(t, shift, "rows", MIN, 0)
    for c in ("sum", "min", "max"):
        assert f[c].dtype == w[c].dtype and np.array_equal(f[c], w[c]), c
    assert np.array_equal(f["count"], w["row"] + 1)
    assert np.array_equal(f["start"], idx - w["row"])
    assert np.array_equal(f["last"], t["payload"])
    # ROWS (MIN, MAX) is the group's row of the group table
    f = F.numpy_frame(t, shift, "rows", MIN, MAX)
    for c in ("start", "count", "sum", "min", "max"):
        assert np.array_equal(f[c], g[c][w["group"]]), c
    if name == "run_length":
        return   # RANGE needs sorted keys inside a group
    # RANGE (0, 0): the key run
    f = F.numpy_frame(t, shift, "range", 0, 0)
    runs = G.numpy_groups(t, 0)
    _, khead = W.heads(t, shift)
    assert np.array_equal(f["count"], runs["count"][np.cumsum(khead) - 1])
    # RANGE (MIN, 0) at i is ROWS (MIN, 0) at i's last peer
    last_peer = f["start"] + f["count"] - 1
    r, rows = F.numpy_frame(t, shift, "range", MIN, 0), F.numpy_frame(t, shift, "rows", MIN, 0)
    for c in F.COLUMNS:
        assert np.array_equal(r[c], rows[c][last_peer]), c


@pytest.mark.parametrize("width", [8, 16])
def test_cases_hold_what_they_promise(width):
    T, BLK, B = F.T, F.BLK, F.B
    assert len(F.CASES) == 102
    for name in F.CASES:
        t, shift, unit, lo, hi = F.inputs(width, name)
        assert t.dtype.itemsize == width and 0 <= shift <= 63 and unit in ("rows", "range")
        assert MIN <= lo <= MAX and MIN <= hi <= MAX and len(t) < 1 << 23
        if unit == "range":   # sorted inside every group
            key = t["key"].astype(np.int64)
            head, _ = W.heads(t, shift)
            assert (np.diff(key)[~head[1:]] >= 0).all(), name
    # ROWS (-2, 1) runs on every relation of group_ref
    assert all(f"rows_m2_1/{n}" in F.CASES for n in G.CASES)
    one = F.inputs(width, "ends_m5_m2/one_key_short")[0]
    assert len(one) == 5 * T + 3 and len(np.unique(one["key"])) == 1
    # the triples: frames of BLK - 1, BLK, BLK + 1 and T - 1, T, T + 1 rows
    widths = sorted(1 - lo for lo, hi in F.ENDS[:6])
    assert widths == [BLK - 1, BLK, BLK + 1, T - 1, T, T + 1]
    for lo, hi in F.ENDS:
        a, b, empty = F.frame_bounds(one, 0, "rows", lo, hi)
        q = ~empty
        same_block, same_tile = a[q] // BLK == b[q] // BLK, a[q] // T == b[q] // T
        if (lo, hi) in F.ALL_EMPTY:
            assert empty.all()
        elif (lo, hi) == (-5, -2):
            i = np.flatnonzero(q)
            assert (same_block & (a[q] // BLK != i // BLK)).any()
        elif (lo, hi) == (-70, 3):
            assert (~same_block & same_tile).any() and (~same_tile).any()
        elif (lo, hi) == (-(3 * T + 7), 2 * T + 1):
            assert (b[q] // T - a[q] // T).max() >= 4     # whole tiles between
        elif (lo, hi) in ((2, 5), (-7, -3)):
            i = np.flatnonzero(q)
            assert ((i < a[q]) | (i > b[q])).all() and empty.any()
    # LAG / LEAD at a group head that is a tile's first element
    t, shift, _, _, _ = F.inputs(width, "lag1/key_head_at_tile_edges")
    head, _ = W.heads(t, shift)
    assert head[2 * T] and not head[2 * T - 1]
    assert F.expected(width, "lag1/key_head_at_tile_edges")["count"][2 * T] == 0
    assert F.expected(width, "lag1/key_head_at_tile_edges")["count"][2 * T - 1] == 1
    assert F.expected(width, "lead1/key_head_at_tile_edges")["count"][2 * T - 1] == 0
    assert F.expected(width, "lead1/key_head_at_tile_edges")["count"][2 * T] == 1
    e = F.expected(width, "lag_other_tile/one_key_short")
    q = e["start"] >= 0
    assert (e["count"][q] == 1).all() and (e["start"][q] // T != np.flatnonzero(q) // T).all()
    # far: more than B tiles in one group; behind dense_resets' far group the
    # short groups do not reach it
    for name in ("one_key_long", "dense_resets"):
        t, shift, _, lo, hi = F.inputs(width, f"far_min_max/{name}")
        h, e, starts, ends = F.group_ends(t, shift)
        assert (ends[0] - starts[0]) // T > B and (lo, hi) == (MIN, MAX)
        assert -F.FAR_FRAMES[2][0] == (B + 1) * T <= ends[0]
    t, shift, _, _, _ = F.inputs(width, "far_min_0/dense_resets")
    h, e, starts, ends = F.group_ends(t, shift)
    assert len(starts) == 41 and (h[starts[1]:] >= starts[1]).all()
    # RANGE: a key run over a whole tile; key runs of about 3 over B + 3 tiles
    t, shift, _, _, _ = F.inputs(width, "range_0_0/peers_cross_tiles")
    a, b, empty = F.frame_bounds(t, shift, "range", 0, 0)
    assert not empty.any() and (a[T:2 * T] < T).all() and (b[T:2 * T] >= 2 * T).all()
    t, shift, _, _, _ = F.inputs(width, "range_0_0/dense_far")
    a, b, empty = F.frame_bounds(t, shift, "range", 0, 0)
    assert len(t) == (B + 2) * T + 3 and 2.5 < (b - a + 1).mean() < 4.5
    for lo, hi in ((3, 7), (-7, -3)):   # the band excludes the row and its peers
        a, b, empty = F.frame_bounds(t, shift, "range", lo, hi)
        i = np.flatnonzero(~empty)
        assert ((i < a[i]) | (i > b[i])).all() and len(i) > len(t) // 2
    assert F.frame_bounds(t, shift, "range", 2, 1)[2].all()
    # shift 0: the frames are the peers only, though the band is wide
    t, shift, unit, lo, hi = F.inputs(width, "range_m300_300/shift0_ranks")
    assert shift == 0 and (lo, hi) == (-300, 300)
    wide, peers = F.numpy_frame(t, 0, "range", lo, hi), F.numpy_frame(t, 0, "range", 0, 0)
    assert all(np.array_equal(wide[c], peers[c]) for c in F.COLUMNS)
    # shift 63: the two signs are two groups
    t, shift, _, _, _ = F.inputs(width, "range_m5_5/shift63")
    assert shift == 63 and len(F.group_ends(t, shift)[2]) == 2
    # the sweep: the lower ends of part B's rows lie about 1000 apart over all
    # of part A, each in another tile than its neighbour's
    t, shift, unit, lo, hi = F.inputs(width, "range_sweep")
    a, b, empty = F.frame_bounds(t, shift, unit, lo, hi)
    A = F.SWEEP_A
    assert len(t) == A + T + 7 and A == (B + 1) * T and len(F.group_ends(t, shift)[2]) == 1
    assert empty[:A].all() and not empty[A:].any()
    assert (np.diff(a[A + 3:]) == 1000).all() and (b[A:] < A).all()
    assert a[A + 3] == 0 and a[-1] > A - 30000
    assert (np.diff(a[A + 3:] // T) >= 0).all() and len(np.unique(a[A + 3:] // T)) > T - 60
    # the ends of the key type: bands that saturate or lie outside int64
    lo_k, hi_k = G.limits(width)
    for d in F.EDGE_DOMAINS:
        t = F.inputs(width, f"edge_{d}_s0_m50_50")[0]
        assert len(t) == 3 * T + 1
        key = t["key"].astype(np.int64)
        assert (key.max() == hi_k) == (d != "bottom") and (key.min() == lo_k) == (d != "top")
        assert ((key >= hi_k - 40) | (key <= lo_k + 40)).all()
    if width == 16:
        top = F.inputs(16, "edge_top_s0_max_max")[0]
        assert F.frame_bounds(top, 0, "range", MAX, MAX)[2][top["key"] > 0].all()
        assert not F.frame_bounds(top, 0, "range", -30, MAX)[2].any()
