"""Grouped aggregation (smj_dev_group_aggregate, smj_dev_group_count,
Library.group_by).

Expected values come from group_ref.numpy_groups; every comparison is
bit-exact, at both widths.  Every call writes into columns with sentinel room
behind their last row, and the input is compared unchanged after it.

The cases (group_ref.CASES) are the smallest that reach each path of the
kernels: a tile is T = 1024 elements, a workgroup of the carry step covers
B = 1024 tiles.  tests/test_group_aggregate_abi.py checks on CPU that they
hold what their descriptions promise.
"""
import numpy as np
import pytest

import group_ref as G
from placement import arena, arena_column, check_guards
from test_gpu_parity import rand_tuples

pytestmark = pytest.mark.gpu

SENTINEL = -77
ROOM = 7
ALL = (True,) * 6


def dtype_of(lib, c):
    import torch
    return torch.int64 if c in ("start", "count", "sum") or lib.width == 16 else torch.int32


def run_group(lib, dT, shift, which=ALL, cap=None, groups=None):
    """dev_group_aggregate into the first `cap` rows of the columns `which`
    selects, each with ROOM more elements behind them; everything past the
    first min(groups, cap) rows must keep its fill.  Returns ({column: host
    rows written}, the return value)."""
    import torch
    cap = groups + ROOM if cap is None else cap
    bufs = {c: torch.full((cap + ROOM,), SENTINEL, dtype=dtype_of(lib, c), device="cuda")
            for c, w in zip(G.COLUMNS, which) if w}
    got = lib.dev_group_aggregate(dT, shift, **{c: b[:cap] for c, b in bufs.items()})
    torch.cuda.synchronize()
    rows = min(got, cap)
    host = {c: b.cpu().numpy() for c, b in bufs.items()}
    for c, h in host.items():
        assert np.all(h[rows:] == SENTINEL), f"{c}: wrote behind row {rows - 1}"
    return {c: h[:rows] for c, h in host.items()}, got


def check(cols, exp, what, rows=None):
    for c, got in cols.items():
        want = exp[c] if rows is None else exp[c][:rows]
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, c)


def counted(lib, dT, shift):
    """dev_group_count twice into a counter that starts at 5."""
    import torch
    m = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    lib.dev_group_count(dT, shift, m)
    one = int(m.item())
    lib.dev_group_count(dT, shift, m)
    return one - 5, int(m.item()) - one


@pytest.mark.parametrize("name", list(G.CASES))
def test_group_aggregate(libs, width, name):
    lib = libs[width]
    t, shift = G.inputs(width, name)
    exp = G.expected(width, name)
    groups = len(exp["key"])
    dT = lib.to_device(t)
    cols, got = run_group(lib, dT, shift, groups=groups)
    assert got == groups, name
    check(cols, exp, name)
    assert lib.dev_group_aggregate(dT, shift) == groups   # the count-only form
    assert counted(lib, dT, shift) == (groups, groups)
    assert np.array_equal(lib.to_host(dT), t)
    if name == "run_length":
        assert got == 3 and cols["key"].tolist() == [1, 2, 1]
    if name == "shift63":
        assert got == 2
    if name == "all_distinct":
        assert got == len(t)


def test_payload_order_is_free(libs, width):
    """The payloads of some run are not ordered: its minimum and maximum are
    neither its first nor its last payload (asserted on the input), and the
    library still finds them."""
    lib = libs[width]
    t, shift = G.inputs(width, "n3Tp1")
    exp = G.expected(width, "n3Tp1")
    first, last = t["payload"][exp["start"]], t["payload"][exp["start"] + exp["count"] - 1]
    inner = (exp["min"] != first) & (exp["min"] != last) & (exp["max"] != first) & \
        (exp["max"] != last)
    assert inner.any()
    cols, _ = run_group(lib, lib.to_device(t), shift, groups=len(first))
    assert np.array_equal(cols["min"][inner], exp["min"][inner])
    assert np.array_equal(cols["max"][inner], exp["max"][inner])


@pytest.mark.parametrize("name", ["n3Tp1", "mid0_to_mid3", "long_groups"])
def test_column_subsets_and_capacity(libs, width, name):
    """Each column alone gives the values of the full call; all NULL gives
    the return value only; out_cap cuts the rows, not the return value."""
    import torch
    lib = libs[width]
    t, shift = G.inputs(width, name)
    exp = G.expected(width, name)
    groups = len(exp["key"])
    dT = lib.to_device(t)
    for c in range(6):
        which = tuple(i == c for i in range(6))
        cols, got = run_group(lib, dT, shift, which, groups=groups)
        assert got == groups and list(cols) == [G.COLUMNS[c]]
        check(cols, exp, (name, G.COLUMNS[c]))
    _, got = run_group(lib, dT, shift, (False,) * 6, groups=groups)
    assert got == groups
    for cap in (0, 1, groups - 1, groups + 7):
        cols, got = run_group(lib, dT, shift, cap=cap)
        assert got == groups, cap
        assert all(len(v) == min(groups, cap) for v in cols.values())
        check(cols, exp, (name, cap), rows=min(groups, cap))
    # min and max without sum, and the position columns without aggregates
    for which in ((False,) * 4 + (True,) * 2, (True,) * 3 + (False,) * 3):
        cols, got = run_group(lib, dT, shift, which, cap=groups - 1)
        assert got == groups
        check(cols, exp, (name, which), rows=groups - 1)
    torch.cuda.synchronize()
    assert np.array_equal(lib.to_host(dT), t)


def test_empty_input(libs, width):
    import torch
    lib = libs[width]
    none = lib.empty(0)
    col = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
    assert lib.dev_group_aggregate(none, 0, start=col) == 0
    assert lib.dev_group_aggregate(none, 5) == 0
    m = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    lib.dev_group_count(none, 0, m)
    torch.cuda.synchronize()
    assert int(m.item()) == 5 and bool((col == SENTINEL).all())


def test_odd_offsets(libs, width):
    """The input at an odd tuple offset of its allocation (8 mod 16 for the
    8-byte library) and every column at an odd element offset, guards around
    all of them."""
    import torch
    lib = libs[width]
    t, shift = G.inputs(width, "n3Tp1")
    exp = G.expected(width, "n3Tp1")
    groups = len(exp["key"])
    ibuf, dT = arena(lib, len(t), 1, fill=t)
    placed = {c: arena_column(lib, groups, off, dtype=dtype_of(lib, c))
              for c, off in zip(G.COLUMNS, (1, 3, 1, 5, 3, 1))}
    cbuf, counter = arena_column(None, 1, 3, dtype=torch.int64)
    counter.fill_(5)
    got = lib.dev_group_aggregate(dT, shift, **{c: v for c, (_, v) in placed.items()})
    lib.dev_group_count(dT, shift, counter)
    torch.cuda.synchronize()
    assert got == groups and int(counter.item()) == 5 + groups
    check({c: v.cpu().numpy() for c, (_, v) in placed.items()}, exp, "odd offsets")
    for c, (buf, view) in placed.items():
        check_guards(buf, view, f"group aggregate: {c}")
    check_guards(ibuf, dT, "group aggregate: input")
    check_guards(cbuf, counter, "group count: counter")
    assert np.array_equal(lib.to_host(dT), t)


def test_side_stream(libs, width):
    """The call runs on a side stream while the default stream is idle; the
    call itself synchronises that stream, an event orders the reads."""
    import torch
    lib = libs[width]
    t, shift = G.inputs(width, "head_last_of_tile")
    exp = G.expected(width, "head_last_of_tile")
    groups = len(exp["key"])
    dT = lib.to_device(t)
    bufs = {c: torch.full((groups + ROOM,), SENTINEL, dtype=dtype_of(lib, c), device="cuda")
            for c in G.COLUMNS}
    m = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        assert lib.stream_ptr() == side.cuda_stream
        got = lib.dev_group_aggregate(dT, shift, **{c: b[:groups] for c, b in bufs.items()})
        lib.dev_group_count(dT, shift, m)
        done.record(side)
    torch.cuda.current_stream().wait_event(done)
    host = {c: b.clone().cpu().numpy() for c, b in bufs.items()}   # on the default stream
    assert got == groups and int(m.clone().item()) == 5 + groups
    for c, h in host.items():
        assert np.all(h[groups:] == SENTINEL), c
    check({c: h[:groups] for c, h in host.items()}, exp, "side stream")
    assert np.array_equal(lib.to_host(dT), t)


def test_workspace_reuse_and_trace(libs, width):
    """A large call, a small one and the large one again on one workspace;
    the kernels of a call by name."""
    import torch
    lib = libs[width]
    first = None
    for name in ("one_key_long", "run_length", "one_key_long"):
        t, shift = G.inputs(width, name)
        exp = G.expected(width, name)
        dT = lib.to_device(t)
        cols, got = run_group(lib, dT, shift, groups=len(exp["key"]))
        assert got == len(exp["key"])
        check(cols, exp, name)
        if name == "one_key_long":
            if first is None:
                first = cols
            else:
                assert all(np.array_equal(first[c], cols[c]) for c in G.COLUMNS)
    lib.trace(True)
    try:
        run_group(lib, dT, shift, groups=1)
        m = torch.zeros(1, dtype=torch.int64, device="cuda")
        lib.dev_group_count(dT, shift, m)
        torch.cuda.synchronize()
        trace = lib.trace_read()
    finally:
        lib.trace(False)
    assert int(m.item()) == 1
    for k, launches in (("k_group_count", 2), ("k_mat_scan", 1), ("k_group_carry", 1),
                        ("k_group_write", 1), ("k_group_total", 1)):
        assert trace.get(k, (0, 0))[1] == launches, (k, trace)


def test_consistent_with_the_joins(libs, oracles, width):
    """The group tables of sorted R and S of a dup x dup input: the sum over
    the common keys of count_R * count_S is the merge-join count, and R's
    start / count are the bounds np.searchsorted gives."""
    import torch
    orc, lib = oracles[width], libs[width]
    R = orc.sort(rand_tuples(width, 3000, 5, -200, 200))
    S = orc.sort(rand_tuples(width, 4000, 6, -200, 220))
    dR, dS = lib.to_device(R), lib.to_device(S)
    gR, nR = run_group(lib, dR, 0, groups=len(np.unique(R["key"])))
    gS, nS = run_group(lib, dS, 0, groups=len(np.unique(S["key"])))
    assert nR == len(gR["key"]) and nS == len(gS["key"])
    _, iR, iS = np.intersect1d(gR["key"], gS["key"], return_indices=True)
    pairs = int((gR["count"][iR] * gS["count"][iS]).sum())
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib.dev_merge_join_count(dR, dS, count)
    torch.cuda.synchronize()
    assert pairs == int(count.item()) == orc.merge_join(R, S) and pairs > len(S)
    lb = np.searchsorted(R["key"], gR["key"], "left")
    ub = np.searchsorted(R["key"], gR["key"], "right")
    assert np.array_equal(gR["start"], lb) and np.array_equal(gR["start"] + gR["count"], ub)
    assert np.array_equal(gR["key"], np.unique(R["key"]))


@pytest.mark.parametrize("shift", [0, 4])
def test_group_by(libs, oracles, width, shift):
    """Library.group_by on an unsorted relation: group_ref on the
    oracle-sorted one; start is the run offsets."""
    import torch
    orc, lib = oracles[width], libs[width]
    t = rand_tuples(width, 3 * G.T + 11, 71, -700, 700)
    exp = G.numpy_groups(orc.sort(t), shift)
    dT = lib.to_device(t)
    out = lib.group_by(dT, shift)
    torch.cuda.synchronize()
    assert len(out) == 6 and all(x.dim() == 1 and x.shape[0] == len(exp["key"]) for x in out)
    got = {c: x.cpu().numpy() for c, x in zip(G.COLUMNS, out)}
    check(got, exp, ("group_by", shift))
    assert np.array_equal(got["start"], np.append(0, np.cumsum(got["count"]))[:-1])
    assert np.array_equal(lib.to_host(dT), t)


def test_group_by_empty(libs, width):
    import torch
    lib = libs[width]
    out = lib.group_by(lib.empty(0))
    assert len(out) == 6 and all(x.shape == (0,) for x in out)
    pdt = torch.int32 if width == 8 else torch.int64
    assert [x.dtype for x in out] == [pdt, torch.int64, torch.int64, torch.int64, pdt, pdt]
