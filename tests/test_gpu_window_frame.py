"""Sliding window frames over a sorted relation (smj_dev_window_frame,
Library.rolling).

Expected values come from frame_ref.numpy_frame; every comparison is bit-exact,
at both widths.  Every call writes into columns with sentinel room behind row
n - 1, and the input is compared unchanged after it.

The cases (frame_ref.CASES) are the smallest shapes at which each path of the
kernels can go wrong: a tile is T = 1024 elements, the inner block of the range
minimum BLK = 64, a workgroup of the scan step covers B = 1024 tiles.
tests/test_window_frame_abi.py checks on CPU that they hold what their
descriptions promise.
"""
import numpy as np
import pytest

import frame_ref as F
import window_ref as W
from placement import arena, arena_column, check_guards
from test_gpu_parity import rand_tuples

pytestmark = pytest.mark.gpu

SENTINEL = -77
ROOM = 7
ALL = (True,) * 7
NONE = (False,) * 7
MIN, MAX = F.MIN, F.MAX
SUBSET_CASES = ("ends_m70_3/one_key_short", "range_m5_5/peers_cross_tiles",
                "lag1/key_head_at_tile_edges")
EDGE = [n for n in F.CASES if n.startswith("edge_")]
SINGLE = [n for n in F.CASES if not n.startswith("edge_")]


def only(*names):
    return tuple(c in names for c in F.COLUMNS)


def dtype_of(lib, c):
    import torch
    return torch.int32 if c in ("min", "max", "first", "last") and lib.width == 8 else torch.int64


def run_frame(lib, dT, shift, unit, lo, hi, which=ALL):
    """dev_window_frame into the columns `which` selects, each with ROOM more
    elements behind row n - 1, which must keep their fill.  Returns {column:
    the n host rows}."""
    import torch
    n = dT.shape[0]
    bufs = {c: torch.full((n + ROOM,), SENTINEL, dtype=dtype_of(lib, c), device="cuda")
            for c, w in zip(F.COLUMNS, which) if w}
    lib.dev_window_frame(dT, shift, unit, lo, hi, **{c: b[:n] for c, b in bufs.items()})
    torch.cuda.synchronize()
    host = {c: b.cpu().numpy() for c, b in bufs.items()}
    for c, h in host.items():
        assert np.all(h[n:] == SENTINEL), f"{c}: wrote behind row {n - 1}"
    return {c: h[:n] for c, h in host.items()}


def check(cols, exp, what):
    for c, got in cols.items():
        want = exp[c]
        assert got.dtype == want.dtype and got.shape == want.shape, (what, c)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError((what, c, len(bad), bad[:4].tolist(), got[bad[:4]].tolist(),
                                  want[bad[:4]].tolist()))


def run_case(lib, width, name):
    t, shift, unit, lo, hi = F.inputs(width, name)
    dT = lib.to_device(t)
    cols = run_frame(lib, dT, shift, unit, lo, hi)
    assert list(cols) == list(F.COLUMNS)
    check(cols, F.expected(width, name), name)
    assert np.array_equal(lib.to_host(dT), t)
    return cols


@pytest.mark.parametrize("name", SINGLE)
def test_frame(libs, width, name):
    cols = run_case(libs[width], width, name)
    if name == "rows_m2_1/run_length":
        assert cols["start"].tolist() == [0, 0, 2, 3] and cols["count"].tolist() == [2, 2, 1, 1]
    if name.split("/")[0] in ("ends_2_1", "ends_max_max", "ends_min_min"):
        assert (cols["start"] == -1).all()
        assert not any(cols[c].any() for c in F.COLUMNS[1:])
    if name == "lag1/key_head_at_tile_edges":
        assert cols["count"][2 * F.T] == 0 and cols["count"][2 * F.T - 1] == 1
    if name == "lead1/key_head_at_tile_edges":
        assert cols["count"][2 * F.T - 1] == 0 and cols["count"][2 * F.T] == 1


@pytest.mark.parametrize("shift", F.EDGE_SHIFTS)
@pytest.mark.parametrize("domain", F.EDGE_DOMAINS)
def test_range_at_the_ends_of_the_key_type(libs, width, domain, shift):
    """Bands that saturate at, or lie wholly outside, int64 (for the 8-byte
    library: int32 keys under lo / hi far beyond int32)."""
    names = [n for n in EDGE if n.startswith(f"edge_{domain}_s{shift}_")]
    assert len(names) == len(F.EDGE_FRAMES)
    for name in names:
        run_case(libs[width], width, name)


@pytest.mark.parametrize("name", SUBSET_CASES)
def test_column_subsets(libs, width, name):
    """Each column alone gives the values of the full call; sum alone, the
    extremes without the sum and the calls without an aggregate reach the other
    forms of the kernels; all NULL writes nothing."""
    import torch
    lib = libs[width]
    t, shift, unit, lo, hi = F.inputs(width, name)
    exp = F.expected(width, name)
    dT = lib.to_device(t)
    for c in F.COLUMNS:
        cols = run_frame(lib, dT, shift, unit, lo, hi, only(c))
        assert list(cols) == [c]
        check(cols, exp, (name, c))
    for which in (only("min", "max"), only("start", "count"), only("first", "last"),
                  only("sum", "max")):
        cols = run_frame(lib, dT, shift, unit, lo, hi, which)
        assert len(cols) == 2
        check(cols, exp, (name, which))
    assert run_frame(lib, dT, shift, unit, lo, hi, NONE) == {}
    torch.cuda.synchronize()
    assert np.array_equal(lib.to_host(dT), t)


def test_all_null_and_empty_input(libs, width):
    """All seven columns NULL, and n == 0 with columns given: nothing is
    written."""
    import torch
    lib = libs[width]
    t, shift = W.inputs(width, "n3Tp1")
    dT = lib.to_device(t)
    near = torch.full((len(t) + ROOM,), SENTINEL, dtype=torch.int64, device="cuda")
    lib.dev_window_frame(dT, shift, "rows", -3, 3)
    lib.dev_window_frame(dT, shift, "range", -3, 3)
    none = lib.empty(0)
    lib.dev_window_frame(none, 0, "rows", None, 0, start=near[:0], sum=near[:0])
    lib.dev_window_frame(none, 5, "range")
    torch.cuda.synchronize()
    assert bool((near == SENTINEL).all())
    assert np.array_equal(lib.to_host(dT), t)


@pytest.mark.parametrize("name", ["range_m5_5/peers_cross_tiles", "ends_m70_3/one_key_short"])
def test_odd_offsets(libs, width, name):
    """The input at an odd tuple offset of its allocation (8 mod 16 for the
    8-byte library) and every column at an odd element offset, guards around
    all of them."""
    import torch
    lib = libs[width]
    t, shift, unit, lo, hi = F.inputs(width, name)
    exp = F.expected(width, name)
    ibuf, dT = arena(lib, len(t), 1, fill=t)
    placed = {c: arena_column(lib, len(t), off, dtype=dtype_of(lib, c))
              for c, off in zip(F.COLUMNS, (1, 3, 1, 5, 3, 1, 7))}
    lib.dev_window_frame(dT, shift, unit, lo, hi, **{c: v for c, (_, v) in placed.items()})
    torch.cuda.synchronize()
    check({c: v.cpu().numpy() for c, (_, v) in placed.items()}, exp, "odd offsets")
    for c, (buf, view) in placed.items():
        check_guards(buf, view, f"window_frame: {c}")
    check_guards(ibuf, dT, "window_frame: input")
    assert np.array_equal(lib.to_host(dT), t)


def test_side_stream(libs, width):
    """The call runs on a side stream while the default stream is idle; it
    does not synchronise, an event orders the reads."""
    import torch
    lib = libs[width]
    name = "range_m5_5/peers_cross_tiles"
    t, shift, unit, lo, hi = F.inputs(width, name)
    exp = F.expected(width, name)
    n = len(t)
    dT = lib.to_device(t)
    bufs = {c: torch.full((n + ROOM,), SENTINEL, dtype=dtype_of(lib, c), device="cuda")
            for c in F.COLUMNS}
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        assert lib.stream_ptr() == side.cuda_stream
        lib.dev_window_frame(dT, shift, unit, lo, hi, **{c: b[:n] for c, b in bufs.items()})
        done.record(side)
    torch.cuda.current_stream().wait_event(done)
    host = {c: b.clone().cpu().numpy() for c, b in bufs.items()}   # on the default stream
    for c, h in host.items():
        assert np.all(h[n:] == SENTINEL), c
    check({c: h[:n] for c, h in host.items()}, exp, "side stream")
    assert np.array_equal(lib.to_host(dT), t)


def test_workspace_reuse_and_trace(libs, width):
    """A large call, a small one and the large one again on one workspace;
    the passes of a call by name."""
    import torch
    lib = libs[width]
    big, small = "far_min_max/dense_resets", "rows_m2_1/run_length"
    want = F.expected(width, big)
    for name in (big, small, big):
        t, shift, unit, lo, hi = F.inputs(width, name)
        dT = lib.to_device(t)
        check(run_frame(lib, dT, shift, unit, lo, hi),
              want if name == big else F.expected(width, name), name)

    def traced(which):
        lib.trace(True)
        try:
            run_frame(lib, dT, shift, unit, lo, hi, which)
            torch.cuda.synchronize()
            return lib.trace_read()
        finally:
            lib.trace(False)

    trace = traced(ALL)
    for k in ("k_frame_build", "k_frame_scan", "k_frame_write"):
        assert trace.get(k, (0, 0))[1] == 1, (k, trace)
    assert not any(k.startswith(("k_window", "k_group")) for k in trace), trace
    trace = traced(only("start", "count", "first", "last"))
    assert "k_frame_build" not in trace, trace
    for k in ("k_frame_scan", "k_frame_write"):
        assert trace.get(k, (0, 0))[1] == 1, (k, trace)


@pytest.mark.parametrize("shift", [0, 4])
def test_consistent_with_the_library(libs, oracles, width, shift):
    """On an oracle-sorted relation of duplicate keys: ROWS (MIN, 0) is
    dev_window, ROWS (MIN, MAX) the group table gathered by dev_window's group
    column, RANGE (0, 0) counts the key runs."""
    import torch
    orc, lib = oracles[width], libs[width]
    R = orc.sort(rand_tuples(width, 3000, 5, -200, 200))
    n = len(R)
    dR = lib.to_device(R)
    pdt = dtype_of(lib, "min")
    win = {c: torch.empty(n, dtype=torch.int64 if c in ("group", "row", "sum") else pdt,
                          device="cuda") for c in ("group", "row", "sum", "min", "max")}
    lib.dev_window(dR, shift, **win)
    torch.cuda.synchronize()
    win = {c: v.cpu().numpy() for c, v in win.items()}
    f = run_frame(lib, dR, shift, "rows", MIN, 0)
    for c in ("sum", "min", "max"):
        assert np.array_equal(f[c], win[c]), c
    assert np.array_equal(f["count"], win["row"] + 1)
    assert np.array_equal(f["start"], np.arange(n) - win["row"])

    def group_table(sh):
        groups = lib.dev_group_aggregate(dR, sh)
        tab = {c: torch.empty(groups, dtype=torch.int64 if c in ("start", "count", "sum") else pdt,
                              device="cuda") for c in ("start", "count", "sum", "min", "max")}
        assert lib.dev_group_aggregate(dR, sh, **tab) == groups
        torch.cuda.synchronize()
        return {c: v.cpu().numpy() for c, v in tab.items()}

    tab = group_table(shift)
    f = run_frame(lib, dR, shift, "rows", MIN, MAX)
    for c in ("start", "count", "sum", "min", "max"):
        assert np.array_equal(f[c], tab[c][win["group"]]), c
    runs = group_table(0)
    kgroup = torch.empty(n, dtype=torch.int64, device="cuda")
    lib.dev_window(dR, 0, group=kgroup)
    f = run_frame(lib, dR, shift, "range", 0, 0, only("count"))
    assert np.array_equal(f["count"], runs["count"][kgroup.cpu().numpy()])
    assert f["count"].max() >= 3


@pytest.mark.parametrize("band", [(-3, 4), (0, 0)])
def test_counts_are_the_band_join_with_itself(libs, oracles, width, band):
    """On non-negative keys in one group (shift 63) the RANGE counts add up to
    the band join of the relation with itself."""
    import torch
    orc, lib = oracles[width], libs[width]
    R = orc.sort(rand_tuples(width, 3000, 6, 0, 400))
    dR = lib.to_device(R)
    f = run_frame(lib, dR, 63, "range", band[0], band[1], only("count"))
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib.dev_band_join_count(dR, dR, band[0], band[1], count)
    torch.cuda.synchronize()
    assert int(f["count"].sum()) == int(count.item()) > len(R)


@pytest.mark.parametrize("unit", ["rows", "range"])
@pytest.mark.parametrize("shift", [0, 4])
def test_library_rolling(libs, oracles, width, shift, unit):
    """Library.rolling on an unsorted relation: numpy_frame of the
    oracle-sorted one, the returned sorted relation included."""
    import torch
    orc, lib = oracles[width], libs[width]
    t = rand_tuples(width, 3 * F.T + 11, 71, -700, 700)
    s = orc.sort(t)
    exp = F.numpy_frame(s, shift, unit, -9, 2)
    dT = lib.to_device(t)
    out = lib.rolling(dT, shift, unit, -9, 2)
    torch.cuda.synchronize()
    assert len(out) == 8 and out[0].shape == (len(t), 2)
    assert all(x.dim() == 1 and x.shape[0] == len(t) for x in out[1:])
    assert np.array_equal(lib.to_host(out[0]), s)
    check({c: x.cpu().numpy() for c, x in zip(F.COLUMNS, out[1:])}, exp, ("rolling", shift))
    assert np.array_equal(lib.to_host(dT), t)


def test_library_rolling_empty(libs, width):
    import torch
    lib = libs[width]
    out = lib.rolling(lib.empty(0), 0, "range", -60, 0)
    assert len(out) == 8 and out[0].shape == (0, 2)
    assert all(x.shape == (0,) for x in out[1:])
    pdt = torch.int32 if width == 8 else torch.int64
    assert [x.dtype for x in out] == [pdt] + [torch.int64] * 3 + [pdt] * 4
