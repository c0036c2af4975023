"""As-of join (smj_dev_asof_join).

Expected values come from asof_ref.numpy_asof over the sorted relations: per
S tuple the position of its partner in sorted R, or -1.  The inputs are
sorted by the oracle, so 8-byte ties follow the packed-word order.  Every
comparison is bit-exact, at both widths.  Every call writes into columns with
sentinel room behind row nS, and the inputs are compared unchanged after it.

The cases (asof_ref.CASES) are the smallest that reach each path of the
kernels: a tile is 512 S elements, the staged window holds 1024 R keys.
tests/test_asof_join_abi.py checks on CPU that they hold what their
descriptions promise.
"""
import numpy as np
import pytest

import asof_ref as A
from band_ref import numpy_band
from test_gpu_parity import rand_tuples

pytestmark = pytest.mark.gpu

SENTINEL = -77
ROOM = 5
ROW0 = 5  # the payloads of row_ids() are 5 + row id


def column(lib, n, fill=SENTINEL, index=False):
    import torch
    dt = torch.int64 if index or lib.width == 16 else torch.int32
    return torch.full((n,), fill, dtype=dt, device="cuda")


def expected_columns(R, r_idx):
    """(r_index, r_payload, r_key) of the partners r_idx: -1 / 0 / 0 for none."""
    hit = r_idx >= 0
    pos = np.where(hit, r_idx, 0)
    if len(R) == 0:
        z = np.zeros(len(r_idx), R["key"].dtype)
        return r_idx, z, z
    return r_idx, np.where(hit, R["payload"][pos], 0), np.where(hit, R["key"][pos], 0)


def run_asof(lib, dR, dS, direction, strict, tol, gsh, which=(True, True, True), count=True):
    """dev_asof_join into the first nS rows of the columns `which` selects
    (r_index, r_payload, r_key), each with ROOM more elements that must keep
    their fill; `matched` starts at 5.  Returns ([host column or None] * 3,
    the matched rows added)."""
    import torch
    nS = dS.shape[0]
    bufs = [column(lib, nS + ROOM, index=(i == 0)) if w else None for i, w in enumerate(which)]
    m = torch.full((1,), 5, dtype=torch.int64, device="cuda") if count else None
    lib.dev_asof_join(dR, dS, direction, strict, tol, gsh,
                      *[b[:nS] if b is not None else None for b in bufs], matched=m)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() if b is not None else None for b in bufs]
    for h in host:
        assert h is None or np.all(h[nS:] == SENTINEL), "wrote behind row nS - 1"
    return [h[:nS] if h is not None else None for h in host], \
        (int(m.item()) - 5 if count else None)


def check(cols, added, R, r_idx, what):
    exp = expected_columns(R, r_idx)
    for got, want, name in zip(cols, exp, ("r_index", "r_payload", "r_key")):
        if got is not None:
            assert np.array_equal(got, want), (what, name)
    if added is not None:
        assert added == int((r_idx >= 0).sum()), what


def unchanged(lib, dR, dS, R, S):
    assert np.array_equal(lib.to_host(dR), R) and np.array_equal(lib.to_host(dS), S)


@pytest.mark.parametrize("name", list(A.CASES))
def test_asof_join(libs, oracles, width, name):
    orc, lib = oracles[width], libs[width]
    R, S = A.inputs(orc, width, name)
    dR, dS = lib.to_device(R), lib.to_device(S)
    for tol, gsh in A.CASES[name][1](width):
        for direction, strict in A.MODES:
            what = (name, width, direction, strict, tol, gsh)
            r_idx = A.expected(orc, width, name, direction, strict, tol, gsh)
            cols, added = run_asof(lib, dR, dS, direction, strict, tol, gsh)
            check(cols, added, R, r_idx, what)
            unchanged(lib, dR, dS, R, S)
            if name == "empty_R":
                assert added == 0 and np.all(cols[0] == -1)
                assert np.all(cols[1] == 0) and np.all(cols[2] == 0)
            if name == "one_one":
                assert added == (0 if strict else 1)
            if len(R) and len(S):   # the definition itself, on what came back
                hit = cols[0] >= 0
                rk, sk = cols[2][hit].astype(object), S["key"][hit].astype(object)
                assert np.array_equal(cols[2][hit], R["key"][cols[0][hit]])
                if direction == "backward":
                    assert np.all(rk < sk if strict else rk <= sk)
                if direction == "forward":
                    assert np.all(rk > sk if strict else rk >= sk)
                if tol is not None:
                    assert np.all(abs(sk - rk) <= tol)
                if gsh:
                    assert np.all((rk >> gsh) == (sk >> gsh))


def test_no_limit_is_uint64_max(libs, oracles, width):
    """tolerance = UINT64_MAX is no limit: the far partners of `ends`."""
    orc, lib = oracles[width], libs[width]
    R, S = A.inputs(orc, width, "ends")
    dR, dS = lib.to_device(R), lib.to_device(S)
    for direction in A.DIRECTIONS:
        r_idx = A.expected(orc, width, "ends", direction, True, None, 0)
        cols, added = run_asof(lib, dR, dS, direction, True, (1 << 64) - 1, 0)
        check(cols, added, R, r_idx, direction)


def row_ids(t):
    t["payload"] = np.arange(len(t)) + ROW0
    return t


def test_equals_join_pairs_unique_R(libs, oracles, width):
    """R's keys unique, backward, not strict, tolerance 0: the matched rows
    are dev_join_pairs' three columns exactly."""
    orc, lib = oracles[width], libs[width]
    rng = np.random.default_rng(21)
    R = rand_tuples(width, 3000, 1)
    R["key"] = rng.permutation(3000) + 1
    R, S = orc.sort(R), orc.sort(rand_tuples(width, 1300, 2, 1, 4001))
    dR, dS = lib.to_device(R), lib.to_device(S)
    total = lib.dev_join_pairs(dR, dS)
    assert 0 < total < len(S) and total == orc.merge_join(R, S)
    pr, ps, pk = (column(lib, total) for _ in range(3))
    assert lib.dev_join_pairs(dR, dS, pr, ps, pk) == total
    (idx, pay, key), added = run_asof(lib, dR, dS, "backward", False, 0, 0)
    hit = idx >= 0
    assert added == total == int(hit.sum())
    assert np.array_equal(pay[hit], pr.cpu().numpy())
    assert np.array_equal(S["payload"][hit], ps.cpu().numpy())
    assert np.array_equal(key[hit], pk.cpu().numpy())
    assert np.all(pay[~hit] == 0) and np.all(key[~hit] == 0)


def test_matched_equals_band_count_nonempty(libs, oracles, width):
    """`dups` with tolerance 4: the backward-matched rows are the S rows with
    a partner in the band (-4, 0), the forward-matched those of (0, 4)."""
    orc, lib = oracles[width], libs[width]
    R, S = A.inputs(orc, width, "dups")
    dR, dS = lib.to_device(R), lib.to_device(S)
    for direction, band in (("backward", (-4, 0)), ("forward", (0, 4))):
        _, s_idx = numpy_band(R["key"], S["key"], *band)
        partner = np.zeros(len(S), bool)
        partner[s_idx] = True
        assert 0 < partner.sum() < len(S)
        (idx, _, _), added = run_asof(lib, dR, dS, direction, False, 4, 0)
        assert np.array_equal(idx >= 0, partner), direction
        assert added == int(partner.sum())
        check([idx, None, None], None, R,
              A.numpy_asof(R["key"], S["key"], direction, False, 4, 0), direction)


def test_null_columns(libs, oracles, width):
    """Each single column alone gives the values of the full call; the count
    form writes nothing; with everything NULL nothing happens."""
    import torch
    orc, lib = oracles[width], libs[width]
    R, S = A.inputs(orc, width, "dups")
    dR, dS = lib.to_device(R), lib.to_device(S)
    for direction, strict in (("backward", False), ("nearest", True)):
        full, added = run_asof(lib, dR, dS, direction, strict, 2, 0)
        check(full, added, R, A.numpy_asof(R["key"], S["key"], direction, strict, 2, 0), direction)
        for c in range(3):
            which = tuple(i == c for i in range(3))
            for count in (True, False):
                cols, n = run_asof(lib, dR, dS, direction, strict, 2, 0, which, count)
                assert np.array_equal(cols[c], full[c]), (direction, c)
                assert n == (added if count else None)
        _, n = run_asof(lib, dR, dS, direction, strict, 2, 0, (False, False, False))
        assert n == added
    lib.dev_asof_join(dR, dS)   # nothing to write, nothing to count
    torch.cuda.synchronize()
    unchanged(lib, dR, dS, R, S)


def test_odd_offset_views_and_side_stream(libs, oracles, width):
    """R and S are slices [1:] of larger buffers and the columns start at
    element 1; the call runs on a side stream, an event is recorded behind it
    and the default stream waits for the event before it reads."""
    import torch
    orc, lib = oracles[width], libs[width]
    R, S = A.inputs(orc, width, "s1025")
    nS = len(S)
    r_idx = A.expected(orc, width, "s1025", "nearest", False, None, 0)
    bR, bS = lib.to_device(np.concatenate([R[:1], R])), lib.to_device(np.concatenate([S[:1], S]))
    dR, dS = bR[1:], bS[1:]
    assert dR.data_ptr() == bR.data_ptr() + width and dR.is_contiguous()
    bufs = [column(lib, 1 + nS + ROOM, index=(i == 0)) for i in range(3)]
    views = [b[1:1 + nS] for b in bufs]
    m = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        assert lib.stream_ptr() == side.cuda_stream
        lib.dev_asof_join(dR, dS, "nearest", False, None, 0, *views, matched=m[1:])
        done.record(side)
    torch.cuda.current_stream().wait_event(done)
    host = [b.clone().cpu().numpy() for b in bufs]   # on the default stream
    counts = m.clone().cpu().numpy()
    for h in host:
        assert h[0] == SENTINEL and np.all(h[1 + nS:] == SENTINEL)
    check([h[1:1 + nS] for h in host], int(counts[1]) - 5, R, r_idx, "side stream")
    assert counts[0] == 5
    unchanged(lib, dR, dS, R, S)
    assert np.array_equal(lib.to_host(bR[:1]), R[:1]) and np.array_equal(lib.to_host(bS[:1]), S[:1])


def test_workspace_reuse_and_trace(libs, oracles, width):
    """wide, dups, wide on one workspace; the kernels of a call by name."""
    import torch
    orc, lib = oracles[width], libs[width]
    first = None
    for name in ("wide", "dups", "wide"):
        R, S = A.inputs(orc, width, name)
        dR, dS = lib.to_device(R), lib.to_device(S)
        cols, added = run_asof(lib, dR, dS, "nearest", False, 50, 0)
        check(cols, added, R, A.expected(orc, width, name, "nearest", False, 50, 0), name)
        if name == "wide":
            if first is None:
                first = cols
            else:
                assert all(np.array_equal(a, b) for a, b in zip(first, cols))
    lib.trace(True)
    try:
        run_asof(lib, dR, dS, "nearest", False, 50, 0)
        torch.cuda.synchronize()
        trace = lib.trace_read()
    finally:
        lib.trace(False)
    assert trace and all(k.startswith("k_asof_") for k in trace), trace
    for k in ("k_asof_bounds", "k_asof_tile", "k_asof_total"):
        assert trace.get(k, (0, 0))[1] == 1, (k, trace)


@pytest.mark.parametrize("name", ["dups", "groups"])
def test_one_call(libs, oracles, width, name):
    """Library.asof_join on shuffled copies whose payloads are distinct row
    ids: sorted S is recoverable from s_payloads."""
    import torch
    orc, lib = oracles[width], libs[width]
    gsh = A.GROUP_SHIFT if name == "groups" else 0
    R, S = (row_ids(t.copy()) for t in A.inputs(orc, width, name))
    R, S = orc.sort(R), orc.sort(S)   # distinct payloads: the one order of the tuples
    rng = np.random.default_rng(3)
    uR, uS = lib.to_device(R[rng.permutation(len(R))]), lib.to_device(S[rng.permutation(len(S))])
    hR, hS = lib.to_host(uR), lib.to_host(uS)
    for direction, strict, tol in (("backward", False, None), ("nearest", True, 300)):
        r_idx, pay, key = expected_columns(R, A.numpy_asof(R["key"], S["key"], direction, strict,
                                                           tol, gsh))
        out = lib.asof_join(uR, uS, direction, strict, tol, gsh, with_keys=True)
        two = lib.asof_join(uR, uS, direction, strict, tol, gsh)
        torch.cuda.synchronize()
        assert len(out) == 5 and len(two) == 3
        assert all(torch.equal(a, b) for a, b in zip(out[:3], two))
        assert out[2].dtype == torch.bool
        sp, rp, mask, sk, rk = (x.cpu().numpy() for x in out)
        assert np.array_equal(sp, S["payload"]) and np.array_equal(sk, S["key"])
        assert np.array_equal(rp, pay) and np.array_equal(rk, key)
        assert np.array_equal(mask, r_idx >= 0) and mask.any()
    assert np.array_equal(lib.to_host(uR), hR) and np.array_equal(lib.to_host(uS), hS)


def test_one_call_empty_sides(libs, oracles, width):
    import torch
    lib = libs[width]
    S = lib.to_device(row_ids(rand_tuples(width, 700, 9, 0, 50)))
    none = lib.empty(0)
    sp, rp, mask, sk, rk = lib.asof_join(none, S, "nearest", with_keys=True)
    torch.cuda.synchronize()
    assert sp.shape == rp.shape == mask.shape == sk.shape == rk.shape == (700,)
    assert not bool(mask.any()) and not bool(rp.any()) and not bool(rk.any())
    assert bool((sk[1:] >= sk[:-1]).all())
    assert sorted(sp.tolist()) == list(range(ROW0, ROW0 + 700))
    out = lib.asof_join(S, none, "forward", with_keys=True)
    assert len(out) == 5 and all(x.shape == (0,) for x in out)
    assert out[2].dtype == torch.bool
    assert len(lib.asof_join(S, none)) == 3
