"""Outer joins of two sorted relations (smj_dev_outer_join,
smj_dev_outer_join_count, Library.outer_join).

Expected values come from outer_ref.numpy_outer over the oracle-sorted inputs
(so 8-byte ties follow the packed-word order); test_outer_join_abi.py checks
that construction against the plain definition.  Every comparison is
bit-exact, on all five columns and at both widths; buffers carry a sentinel
past the capacity and it must survive.

The cases (outer_ref.CASES) are the smallest that cross each boundary of the
kernels' geometry: 512-element S tiles, a 1024-key R window, 8192-row work
items.
"""
import numpy as np
import pytest

import outer_ref as O
from placement import arena, arena_column, check_guards

pytestmark = pytest.mark.gpu

SENTINEL = -77
ROOM = 5


def dtype_of(lib, col):
    import torch
    if col in ("r_index", "s_index"):
        return torch.int64
    return torch.int32 if lib.width == 8 else torch.int64


def run_outer(lib, dR, dS, how, cap, which=O.COLUMNS, room=ROOM):
    """dev_outer_join into the first `cap` elements of the columns `which`,
    each with `room` more elements that must keep their fill.  Returns the
    total and the host columns."""
    import torch
    bufs = {c: torch.full((cap + room,), SENTINEL, dtype=dtype_of(lib, c), device="cuda")
            for c in which}
    total = lib.dev_outer_join(dR, dS, how, **{c: b[:cap] for c, b in bufs.items()})
    torch.cuda.synchronize()
    host = {c: b.cpu().numpy() for c, b in bufs.items()}
    for c, h in host.items():
        assert np.all(h[cap:] == SENTINEL), f"{c}: wrote past the capacity"
    return total, {c: h[:cap] for c, h in host.items()}


def check_rows(cols, exp, rows, what, rest=SENTINEL):
    """The first `rows` rows of every column equal the expected ones; what
    lies behind them inside the capacity was left alone."""
    for c, got in cols.items():
        assert np.array_equal(got[:rows], exp[c][:rows]), (what, c)
        assert np.all(got[rows:] == rest), (what, c, "rows past the total")


@pytest.mark.parametrize("name", list(O.CASES))
def test_outer_join(libs, oracles, width, name):
    import torch
    orc, lib = oracles[width], libs[width]
    R, S = O.inputs(orc, width, name)
    dR, dS = lib.to_device(R), lib.to_device(S)
    totals, got = {}, {}
    for how in O.HOWS:
        r_idx, s_idx, key = O.expected(orc, width, name, how)
        exp = O.expected_columns(R, S, r_idx, s_idx, key)
        total = len(r_idx)
        assert lib.dev_outer_join(dR, dS, how) == total, how  # count only
        counter = torch.full((1,), 3, dtype=torch.int64, device="cuda")
        lib.dev_outer_join_count(dR, dS, how, counter)
        t, cols = run_outer(lib, dR, dS, how, total + 2)
        assert t == total and int(counter.item()) == 3 + total, how
        check_rows(cols, exp, total, (name, how))
        assert np.all(np.diff(cols["key_out"][:total].astype(np.int64)) >= 0), how
        # column subsets give the same values
        for which in (("r_index", "s_index"), ("key_out",)):
            t, sub = run_outer(lib, dR, dS, how, total, which)
            assert t == total
            for c in which:
                assert np.array_equal(sub[c], cols[c][:total]), (how, which, c)
        totals[how], got[how] = total, {c: v[:total] for c, v in cols.items()}
    # inner: dev_join_pairs, column for column
    n = totals["inner"]
    pr, ps, pk = (torch.full((n + ROOM,), SENTINEL, dtype=dtype_of(lib, "r_out"), device="cuda")
                  for _ in range(3))
    assert lib.dev_join_pairs(dR, dS, pr[:n], ps[:n], pk[:n]) == n
    torch.cuda.synchronize()
    for c, p in (("r_out", pr), ("s_out", ps), ("key_out", pk)):
        assert np.array_equal(got["inner"][c], p.cpu().numpy()[:n]), c
    # right: the rows without an R tuple are the anti join of S, in order;
    # left: those without an S tuple the anti join with the arguments swapped
    anti = {}
    for how, side, (A, B), T in (("right", "r_index", (dR, dS), S), ("left", "s_index", (dS, dR), R)):
        m = lib.dev_semi_join(A, B, anti=True)
        out = lib.empty(m)
        assert lib.dev_semi_join(A, B, out, anti=True) == m
        torch.cuda.synchronize()
        out = lib.to_host(out)
        lone = got[how][side] == -1
        other = "s" if how == "right" else "r"
        assert int(lone.sum()) == m, how
        assert np.array_equal(got[how][other + "_out"][lone], out["payload"])
        assert np.array_equal(got[how]["key_out"][lone], out["key"])
        assert np.array_equal(T[got[how][other + "_index"][lone]], out)
        anti[how] = m
    assert totals["full"] == n + anti["left"] + anti["right"]
    assert totals["left"] == n + anti["left"] and totals["right"] == n + anti["right"]
    # full: every position of R and of S occurs
    for c, T in (("r_index", R), ("s_index", S)):
        seen = np.unique(got["full"][c])
        assert np.array_equal(seen[seen >= 0], np.arange(len(T))), c
    torch.cuda.synchronize()
    if len(R):
        assert np.array_equal(lib.to_host(dR), R)
    if len(S):
        assert np.array_equal(lib.to_host(dS), S)


def hot_cap(key):
    """ends inside the hot key's pairs"""
    return int(np.argmax(key == 777)) + 900_000 // 3 + 17


@pytest.mark.parametrize("name,how,cap", [
    ("hot", "full", hot_cap), ("hot", "inner", hot_cap),
    ("r_gaps", "full", lambda key: 9000 // 2 + 17),            # inside the leading R-only run
    ("r_gaps", "left", lambda key: 9000 + 2 + 9000 // 2 + 17),  # inside the inner one
    ("r_gaps", "full", lambda key: 9000 + 2 + 9000 + 2 + 8192 + 5),  # the trailing one
], ids=["hot_full", "hot_inner", "gap_lead", "gap_inner", "gap_trail"])
def test_capacity(libs, oracles, width, name, how, cap):
    """A short buffer receives the prefix, the sentinel behind it survives and
    the total is still returned."""
    orc, lib = oracles[width], libs[width]
    R, S = O.inputs(orc, width, name)
    r_idx, s_idx, key = O.expected(orc, width, name, how)
    cap = cap(key)
    exp = O.expected_columns(R, S, r_idx, s_idx, key)
    assert 0 < cap < len(r_idx)
    row = (r_idx[cap], s_idx[cap])   # the first row cut off
    if name == "hot":
        assert R["key"][row[0]] == 777 and S["key"][row[1]] == 777
    else:
        assert row[1] == -1 and R["key"][row[0]] == R["key"][r_idx[cap - 1]]
    dR, dS = lib.to_device(R), lib.to_device(S)
    total, cols = run_outer(lib, dR, dS, how, cap, room=20000)
    assert total == len(r_idx)
    check_rows(cols, exp, cap, (name, how, cap))


def test_total_above_2_32(libs, oracles, width):
    """70 000 x 70 000 on key 42 between 5 R-only and 5 S-only tuples: the
    total needs 64 bits."""
    import torch
    orc, lib = oracles[width], libs[width]
    n = 70_000
    R = O.fixed(width, 17, [41] * 5 + [42] * n)
    S = O.fixed(width, 18, [42] * n + [43] * 5)
    R, S = orc.sort(R), orc.sort(S)
    dR, dS = lib.to_device(R), lib.to_device(S)
    want = n * n + 10
    assert lib.dev_outer_join(dR, dS, "full") == want
    counter = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    lib.dev_outer_join_count(dR, dS, "full", counter)
    total, cols = run_outer(lib, dR, dS, "full", 1000)
    assert total == want and int(counter.item()) == 3 + want
    r_idx = np.r_[np.arange(5), np.full(995, 5)]
    s_idx = np.r_[np.full(5, -1), np.arange(995)]
    key = np.r_[np.full(5, 41), np.full(995, 42)]
    check_rows(cols, O.expected_columns(R, S, r_idx, s_idx, key), 1000, "above 2^32")
    assert lib.dev_outer_join(dR, dS, "inner") == n * n
    assert lib.dev_outer_join(dR, dS, "left") == n * n + 5


@pytest.mark.parametrize("name", ["dups", "r_gaps", "empty_S"])
def test_odd_offset_views(libs, oracles, name):
    """8-byte tuples: the inputs are slices at an address that is 8 mod 16 and
    every column is a view at an odd element offset, guards around all."""
    import torch
    orc, lib = oracles[8], libs[8]
    R, S = O.inputs(orc, 8, name)
    r_idx, s_idx, key = O.expected(orc, 8, name, "full")
    exp = O.expected_columns(R, S, r_idx, s_idx, key)
    total = len(r_idx)
    rbuf, dR = arena(lib, len(R), 1, fill=R)
    sbuf, dS = arena(lib, len(S), 3, fill=S)
    placed = {c: arena_column(lib, total, off, dtype=dtype_of(lib, c))
              for c, off in zip(O.COLUMNS, (1, 3, 1, 5, 3))}
    cbuf, counter = arena_column(None, 1, 3, dtype=torch.int64)
    counter.fill_(3)
    got = lib.dev_outer_join(dR, dS, "full", **{c: v for c, (_, v) in placed.items()})
    lib.dev_outer_join_count(dR, dS, "full", counter)
    torch.cuda.synchronize()
    assert got == total and int(counter.item()) == 3 + total
    for c, (buf, view) in placed.items():
        assert np.array_equal(view.cpu().numpy(), exp[c]), c
        check_guards(buf, view, f"outer join: {c}")
    check_guards(rbuf, dR, "outer join: R")
    check_guards(sbuf, dS, "outer join: S")
    check_guards(cbuf, counter, "outer join count: counter")


def one_call(lib, orc, R, S):
    import torch
    Rs, Ss = orc.sort(lib.to_host(R)), orc.sort(lib.to_host(S))
    n = R.shape[0]
    for how in O.HOWS:
        cols = lib.outer_join(R, S, how, with_keys=True)
        four = lib.outer_join(R, S, how, key_range=(1, 2 * n))
        torch.cuda.synchronize()
        r_idx, s_idx, key = O.numpy_outer(Rs["key"], Ss["key"], O.KEEP[how])
        exp = O.expected_columns(Rs, Ss, r_idx, s_idx, key)
        assert len(cols) == 5 and len(four) == 4
        for c, got, again in zip(O.COLUMNS, cols, four + (None,)):
            assert got.dtype == dtype_of(lib, c) and got.shape == (len(r_idx),), (how, c)
            assert np.array_equal(got.cpu().numpy(), exp[c]), (how, c)
            assert again is None or torch.equal(got, again), (how, c)


def test_one_call_pk_fk(libs, oracles, width):
    """outer_join on unsorted device relations: S is n of the 2n keys 1..2n,
    so about half of each side has no partner."""
    orc, lib = oracles[width], libs[width]
    n = 1 << 16
    R, S = lib.empty(n), lib.empty(n)
    lib.dev_gen_pk(R, 0, n, 12345)
    lib.dev_gen_fk(S, 0, 2 * n, 2 * n, 54321)
    matched = int((S[:, 1] <= n).sum().item())
    assert n // 4 < matched < 3 * n // 4
    one_call(lib, orc, R, S)


def test_one_call_zipf(libs, oracles, width):
    orc, lib = oracles[width], libs[width]
    n = 1 << 16
    R, S = lib.empty(n), lib.empty(n)
    lib.dev_gen_pk(R, 0, n, 12345)
    lib.dev_gen_zipf(S, 0, n, 0.75, 777)
    one_call(lib, orc, R, S)


def test_one_call_empty_sides(libs, width):
    import torch
    lib = libs[width]
    R, none = lib.empty(100), lib.empty(0)
    lib.dev_gen_pk(R, 0, 100, 7)
    r, s, rp, sp, k = lib.outer_join(R, none, "left", with_keys=True)
    torch.cuda.synchronize()
    assert r.tolist() == list(range(100)) and bool((s == -1).all()) and bool((sp == 0).all())
    assert k.tolist() == list(range(1, 101))
    assert all(len(c) == 0 for c in lib.outer_join(R, none, "right"))
    assert all(len(c) == 0 for c in lib.outer_join(none, none, "full"))
    r, s, rp, sp = lib.outer_join(none, R, "full")
    torch.cuda.synchronize()
    assert s.tolist() == list(range(100)) and bool((r == -1).all()) and bool((rp == 0).all())
