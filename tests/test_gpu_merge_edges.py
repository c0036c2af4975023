"""The merge kernels (csrc/mergesort.hip) at tile edges, key extremes and LDS
overflow: the cases of merge_ref.py through the device entry points
dev_merge2, dev_multiway_merge and dev_merge_join_count, at both widths.

Every output lies in an arena with guards on both sides (placement.py), filled
with a sentinel tuple that is in no input, so a slot nobody wrote shows up.  A
k-way case first asserts the library's record of what it did
(Library.merge_stats: form, k, D and the buckets queued for k_km_over) against
merge_ref.decide, then compares bit-exactly with the numpy reference, then
checks the guards and that the inputs are unchanged.  A third of the cases
also goes through the host entry points (avx_merge_tuples, avx_multiway_merge,
merge_join), which copy and call the same kernels.
tests/test_merge_cases.py checks on the CPU that the cases hold what they
promise and that the reference is the oracle's.
"""
import numpy as np
import pytest

import merge_ref as M
from placement import arena, check_guards

pytestmark = pytest.mark.gpu

GUARD_WORD = -0x1234567


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        unwritten = int(((got["key"] == M.SENTINEL) & (got["payload"] == M.SENTINEL)).sum())
        raise AssertionError((what, f"{len(bad)} of {len(want)} differ, {unwritten} unwritten",
                              bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()))


def merged_into_arena(lib, call, inputs, exp, off, what):
    """call(device inputs, out) into a guarded, sentinel-filled arena at tuple
    offset `off`; the output, the guards and the inputs are checked."""
    import torch
    dev = [lib.to_device(t) for t in inputs]
    buf, out = arena(lib, len(exp), off)
    call(dev, out)
    torch.cuda.synchronize()
    return dev, buf, out


def finish(lib, dev, buf, out, inputs, exp, what):
    got = lib.to_host(out) if len(exp) else np.zeros(0, lib.dtype)
    same(got, exp, what)
    check_guards(buf, out, what)
    for d, t in zip(dev, inputs):
        if len(t):
            assert np.array_equal(lib.to_host(d), t), (what, "an input changed")


TWO_WAY = [(c, n) for c in M.CONTENTS for n in M.SIZES2]


@pytest.mark.parametrize("content,n", TWO_WAY, ids=[f"{c}-{n}" for c, n in TWO_WAY])
def test_merge2(libs, width, content, n):
    """k_mergetile: la + lb around one and two tiles, every split, every
    content (five cases a test)."""
    lib = libs[width]
    if content not in M.contents(width):
        assert width == 16 and content == "sign_straddle"   # the 8-byte packed word's case
        return
    for i, sp in enumerate(M.SPLITS):
        a, b, exp = M.two_way_inputs(width, content, n, sp)
        what = (content, n, sp)
        idx = TWO_WAY.index((content, n)) * len(M.SPLITS) + i
        dev, buf, out = merged_into_arena(lib, lambda d, o: lib.dev_merge2(d[0], d[1], o),
                                          [a, b], exp, idx % 2, what)
        finish(lib, dev, buf, out, [a, b], exp, what)
        if idx % 3 == 0:
            same(lib.avx_merge_tuples(a, b), exp, what + ("avx_merge_tuples",))


KWAY = list(M.KWAY)


@pytest.mark.parametrize("name", KWAY)
def test_multiway_merge(libs, width, name):
    """k_km_bounds, k_km_merge and k_km_over, or the tree of k_mergetile
    passes: the record first, then the output."""
    lib = libs[width]
    runs, promise = M.kway_inputs(width, name)
    exp = M.kway_expected(width, name)
    dec = M.decide(width, runs)
    idx = KWAY.index(name)
    dev, buf, out = merged_into_arena(lib, lib.dev_multiway_merge, runs, exp, idx % 2, name)
    rec = lib.merge_stats()
    assert rec == M.record_of(dec), (name, rec, M.record_of(dec))
    assert rec["form"] == promise["form"] and rec["k"] == len(runs)
    if rec["form"] == "buckets":
        assert (rec["D"], rec["queued"]) == (promise["D"], promise["queued"]), (name, rec)
    finish(lib, dev, buf, out, runs, exp, name)
    if idx % 3 == 0:
        got, n, consumed = lib.avx_multiway_merge(runs)
        assert n == len(exp) and consumed
        same(got, exp, (name, "avx_multiway_merge"))


def test_merge_stats_binding_and_first_call(libs, width):
    """The record is -1 (None) before the first k-way merge on a workspace; a
    2-way merge (the calling thread's workspace) leaves it alone; a merge of
    no tuples and a tree merge replace what a one-pass merge left."""
    import smj
    import torch
    assert smj.MERGE_STATS == ("form", "k", "D", "queued")
    assert smj.MERGE_FORMS == ("none", "buckets", "tree")
    assert "smj_workspace_merge_stats" in smj.DEVICE_SYMBOLS
    lib = smj.Library(width)
    try:
        assert lib.merge_stats() is None
        a, b, exp = M.two_way_inputs(width, "interleaved", M.MG_TILE + 1, "half")
        da, db, out = lib.to_device(a), lib.to_device(b), lib.empty(len(exp))
        lib.dev_merge2(da, db, out)
        torch.cuda.synchronize()
        assert lib.merge_stats() is None
        for name in ("one_key_cap_p1", "no_tuples", "two_hot", "tree_k1_n1"):
            runs, _ = M.kway_inputs(width, name)
            out = lib.empty(sum(len(r) for r in runs))
            lib.dev_multiway_merge([lib.to_device(r) for r in runs], out)
            torch.cuda.synchronize()
            assert lib.merge_stats() == M.record_of(M.decide(width, runs)), name
    finally:
        lib.reset_workspace()


@pytest.mark.parametrize("name", list(M.COUNTS))
def test_merge_join_count(libs, width, name):
    """k_mjcount adds onto a counter that starts at COUNTER_START; its
    neighbours and the inputs stay as they were."""
    import torch
    lib = libs[width]
    r, s, exp = M.count_inputs(width, name)
    dr, ds = lib.to_device(r), lib.to_device(s)
    cnt = torch.tensor([GUARD_WORD, M.COUNTER_START, GUARD_WORD], dtype=torch.int64,
                       device="cuda")
    lib.dev_merge_join_count(dr, ds, cnt[1:2])
    torch.cuda.synchronize()
    got = [int(x) for x in cnt.cpu().numpy().view(np.uint64)]
    assert got[1] == M.COUNTER_START + exp, (name, got[1] - M.COUNTER_START, exp)
    assert got[0] == got[2] == GUARD_WORD % (1 << 64)
    for d, t in ((dr, r), (ds, s)):
        if len(t):
            assert np.array_equal(lib.to_host(d), t)
    if list(M.COUNTS).index(name) % 3 == 0:
        assert lib.merge_join(r, s) == exp
