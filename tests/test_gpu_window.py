"""Window functions over a sorted relation (smj_dev_window, Library.window).

Expected values come from window_ref.numpy_window; every comparison is
bit-exact, at both widths.  Every call writes into columns with sentinel room
behind row n - 1, and the input is compared unchanged after it.

The cases (window_ref.CASES) are group_ref's and the smallest that reach each
path of the key level: a tile is T = 1024 elements, a workgroup of the carry
step covers B = 1024 tiles.  tests/test_window_abi.py checks on CPU that they
hold what their descriptions promise.
"""
import numpy as np
import pytest

import window_ref as W
from placement import arena, arena_column, check_guards
from test_gpu_parity import rand_tuples

pytestmark = pytest.mark.gpu

SENTINEL = -77
ROOM = 7
ALL = (True,) * 7
NONE = (False,) * 7
SUBSET_CASES = ("n3Tp1", "peers_cross_tiles", "dense_far")


def only(*names):
    return tuple(c in names for c in W.COLUMNS)


def dtype_of(lib, c):
    import torch
    return torch.int32 if c in ("min", "max") and lib.width == 8 else torch.int64


def run_window(lib, dT, shift, which=ALL):
    """dev_window into the columns `which` selects, each with ROOM more
    elements behind row n - 1, which must keep their fill.  Returns {column:
    the n host rows}."""
    import torch
    n = dT.shape[0]
    bufs = {c: torch.full((n + ROOM,), SENTINEL, dtype=dtype_of(lib, c), device="cuda")
            for c, w in zip(W.COLUMNS, which) if w}
    lib.dev_window(dT, shift, **{c: b[:n] for c, b in bufs.items()})
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


@pytest.mark.parametrize("name", list(W.CASES))
def test_window(libs, width, name):
    lib = libs[width]
    t, shift = W.inputs(width, name)
    exp = W.expected(width, name)
    dT = lib.to_device(t)
    cols = run_window(lib, dT, shift)
    assert list(cols) == list(W.COLUMNS)
    check(cols, exp, name)
    assert np.array_equal(lib.to_host(dT), t)
    if name == "run_length":
        assert cols["group"].tolist() == [0, 0, 1, 2] and cols["row"].tolist() == [0, 1, 0, 0]
    if name == "shift0_ranks":
        assert not cols["rank"].any() and not cols["dense_rank"].any() and cols["row"].any()
    if name == "dense_far":
        assert cols["dense_rank"][-1] > len(t) // 4


@pytest.mark.parametrize("name", SUBSET_CASES)
def test_column_subsets(libs, width, name):
    """Each column alone gives the values of the full call; row and sum, the
    extremes without the sum and the ranks without aggregates reach the other
    forms of the kernels; all NULL writes nothing."""
    import torch
    lib = libs[width]
    t, shift = W.inputs(width, name)
    exp = W.expected(width, name)
    dT = lib.to_device(t)
    for c in W.COLUMNS:
        cols = run_window(lib, dT, shift, only(c))
        assert list(cols) == [c]
        check(cols, exp, (name, c))
    for which in (only("row", "sum"), only("min", "max"), only("rank", "dense_rank"),
                  only("group", "rank"), only("dense_rank", "sum")):
        cols = run_window(lib, dT, shift, which)
        assert len(cols) == 2
        check(cols, exp, (name, which))
    assert run_window(lib, dT, shift, NONE) == {}
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
    lib.dev_window(dT, shift)
    none = lib.empty(0)
    lib.dev_window(none, 0, row=near[:0], sum=near[:0])
    lib.dev_window(none, 5)
    torch.cuda.synchronize()
    assert bool((near == SENTINEL).all())
    assert np.array_equal(lib.to_host(dT), t)


def test_odd_offsets(libs, width):
    """The input at an odd tuple offset of its allocation (8 mod 16 for the
    8-byte library) and every column at an odd element offset, guards around
    all of them."""
    import torch
    lib = libs[width]
    t, shift = W.inputs(width, "peers_cross_tiles")
    exp = W.expected(width, "peers_cross_tiles")
    ibuf, dT = arena(lib, len(t), 1, fill=t)
    placed = {c: arena_column(lib, len(t), off, dtype=dtype_of(lib, c))
              for c, off in zip(W.COLUMNS, (1, 3, 1, 5, 3, 1, 7))}
    lib.dev_window(dT, shift, **{c: v for c, (_, v) in placed.items()})
    torch.cuda.synchronize()
    check({c: v.cpu().numpy() for c, (_, v) in placed.items()}, exp, "odd offsets")
    for c, (buf, view) in placed.items():
        check_guards(buf, view, f"window: {c}")
    check_guards(ibuf, dT, "window: input")
    assert np.array_equal(lib.to_host(dT), t)


def test_side_stream(libs, width):
    """The call runs on a side stream while the default stream is idle; it
    does not synchronise, an event orders the reads."""
    import torch
    lib = libs[width]
    t, shift = W.inputs(width, "key_head_at_tile_edges")
    exp = W.expected(width, "key_head_at_tile_edges")
    n = len(t)
    dT = lib.to_device(t)
    bufs = {c: torch.full((n + ROOM,), SENTINEL, dtype=dtype_of(lib, c), device="cuda")
            for c in W.COLUMNS}
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        assert lib.stream_ptr() == side.cuda_stream
        lib.dev_window(dT, shift, **{c: b[:n] for c, b in bufs.items()})
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
    first = None
    for name in ("dense_far", "run_length", "dense_far"):
        t, shift = W.inputs(width, name)
        dT = lib.to_device(t)
        cols = run_window(lib, dT, shift)
        check(cols, W.expected(width, name), name)
        if name == "dense_far":
            if first is None:
                first = cols
            else:
                assert all(np.array_equal(first[c], cols[c]) for c in W.COLUMNS)
    lib.trace(True)
    try:
        run_window(lib, dT, shift)
        torch.cuda.synchronize()
        trace = lib.trace_read()
    finally:
        lib.trace(False)
    for k in ("k_window_count", "k_mat_scan", "k_window_carry", "k_window_write"):
        assert trace.get(k, (0, 0))[1] == 1, (k, trace)
    assert not any(k.startswith("k_group") for k in trace), trace


@pytest.mark.parametrize("shift", [0, 4])
def test_consistent_with_the_library(libs, oracles, width, shift):
    """On an oracle-sorted relation of duplicate keys: the group table
    gathered with the group column, at each group's last tuple, is the
    window's running values there; rank plus the group's start is the first
    position of the tuple's key."""
    import torch
    orc, lib = oracles[width], libs[width]
    R = orc.sort(rand_tuples(width, 3000, 5, -200, 200))
    n = len(R)
    dR = lib.to_device(R)
    win = run_window(lib, dR, shift)
    groups = int(win["group"][-1]) + 1
    pdt = dtype_of(lib, "min")
    tab = {c: torch.empty(groups, dtype=torch.int64 if c in ("start", "count", "sum") else pdt,
                          device="cuda") for c in ("start", "count", "sum", "min", "max")}
    assert lib.dev_group_aggregate(dR, shift, **tab) == groups
    torch.cuda.synchronize()
    tab = {c: v.cpu().numpy() for c, v in tab.items()}
    last = np.append(np.flatnonzero(np.diff(win["group"])), n - 1)
    assert len(last) == groups and groups > 20
    g = win["group"][last]
    assert np.array_equal(g, np.arange(groups))
    for c in ("sum", "min", "max"):
        assert np.array_equal(tab[c][g], win[c][last]), c
    assert np.array_equal(tab["count"][g], win["row"][last] + 1)
    assert np.array_equal(tab["start"][win["group"]] + win["row"], np.arange(n))
    assert np.array_equal(win["rank"] + tab["start"][win["group"]],
                          np.searchsorted(R["key"], R["key"], "left"))
    assert (win["rank"].any(), win["dense_rank"].any()) == (shift != 0,) * 2


@pytest.mark.parametrize("shift", [0, 4])
def test_library_window(libs, oracles, width, shift):
    """Library.window on an unsorted relation: numpy_window of the
    oracle-sorted one, the returned sorted relation included."""
    import torch
    orc, lib = oracles[width], libs[width]
    t = rand_tuples(width, 3 * W.T + 11, 71, -700, 700)
    s = orc.sort(t)
    exp = W.numpy_window(s, shift)
    dT = lib.to_device(t)
    out = lib.window(dT, shift)
    torch.cuda.synchronize()
    assert len(out) == 8 and out[0].shape == (len(t), 2)
    assert all(x.dim() == 1 and x.shape[0] == len(t) for x in out[1:])
    assert np.array_equal(lib.to_host(out[0]), s)
    check({c: x.cpu().numpy() for c, x in zip(W.COLUMNS, out[1:])}, exp, ("window", shift))
    assert np.array_equal(lib.to_host(dT), t)


def test_library_window_empty(libs, width):
    import torch
    lib = libs[width]
    out = lib.window(lib.empty(0))
    assert len(out) == 8 and out[0].shape == (0, 2)
    assert all(x.shape == (0,) for x in out[1:])
    pdt = torch.int32 if width == 8 else torch.int64
    assert [x.dtype for x in out] == [pdt] + [torch.int64] * 5 + [pdt, pdt]
