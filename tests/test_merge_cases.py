"""The merge cases of merge_ref.py on the CPU: every case holds what its
description promises (by merge_ref.decide, the restatement of the k-way merge's
host decision, and by its tuples), and the numpy reference equals the oracle's
merge, multiway_merge and merge_join on every case and, on all but the largest,
a plain Python loop.  tests/test_gpu_merge_edges.py runs the library on the
same cases.
"""
import numpy as np
import pytest

import merge_ref as M

WIDTHS = [8, 16]


def no_sentinel(arrays):
    for t in arrays:
        assert not ((t["key"] == M.SENTINEL) & (t["payload"] == M.SENTINEL)).any()


def is_sorted(t):
    return np.array_equal(t, M.srt(t))


def test_geometry_matches_the_source():
    """The constants the cases are built from are the kernels'."""
    import os
    import re
    from conftest import PKG
    src = open(os.path.join(PKG, "csrc", "mergesort.hip")).read()

    def const(name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1).strip()
    assert const("MG_TILE").startswith(str(M.MG_TILE))
    assert const("KM_CAP") == "sizeof(Tup) == 8 ? %d : %d" % (M.cap(8), M.cap(16))
    assert const("KM_KMAX") == "KM_THREADS" and const("KM_THREADS") == str(M.KM_KMAX)
    assert const("KM_LOGNB").startswith(str(M.KM_LOGNB))
    assert const("KM_RUNMAX").startswith(str(M.KM_RUNMAX))
    assert "if (blocks > 4096) blocks = 4096;" in src and M.MJ_GRID == 4096 * 256
    assert "if (k < 3 || k > KM_KMAX) return false;" in src
    assert "(total >> D) > KM_CAP / 2" in src


def test_merge_stats_is_declared_and_bound():
    """smj_merge_stats and SMJ_MERGE_* of smj.h against the binding's names;
    both libraries export the accessor (no device call here)."""
    import ctypes
    import os
    import re
    import smj
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "smj.h")).read()
    body = re.search(r"typedef struct smj_merge_stats \{(.*?)\} smj_merge_stats;", hdr, re.S)
    fields = re.findall(r"uint32_t (\w+);", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S))
    assert tuple(fields) == smj.MERGE_STATS
    forms = {n.lower(): int(v) for n, v in re.findall(r"#define SMJ_MERGE_(\w+)\s+(\d+)u", hdr)}
    assert forms == {n: i for i, n in enumerate(smj.MERGE_FORMS)}
    assert "smj_workspace_merge_stats" in smj.DEVICE_SYMBOLS
    if not all(os.path.exists(smj.lib_path(w)) for w in WIDTHS):
        smj.build()
    for w in WIDTHS:
        assert hasattr(ctypes.CDLL(smj.lib_path(w)), "smj_workspace_merge_stats")
        assert callable(smj.Library(w).merge_stats)


@pytest.mark.parametrize("width", WIDTHS)
def test_order_of_the_packed_word(width):
    """srt against sorting the tuples' bytes as what the kernels compare: the
    signed 64-bit word at 8 bytes, (key, payload) at 16."""
    t = M.rand_tuples(width, 3000, 1, -3, 3)
    s = M.srt(t)
    if width == 8:
        assert np.array_equal(s.view(np.int64), np.sort(t.view(np.int64)))
        one = s[s["key"] == 0]["payload"]
        assert one[0] >= 0 > one[-1]
    else:
        py = sorted(zip(t["key"].tolist(), t["payload"].tolist()))
        assert list(zip(s["key"].tolist(), s["payload"].tolist())) == py


@pytest.mark.parametrize("content", M.CONTENTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_two_way_cases(oracles, width, content):
    if content not in M.contents(width):
        assert width == 16 and content == "sign_straddle"
        return
    orc = oracles[width]
    for n in M.SIZES2:
        seen = set()
        for sp in M.SPLITS:
            a, b, exp = M.two_way_inputs(width, content, n, sp)
            assert (len(a), len(b)) == M.split(n, sp) and len(a) + len(b) == n
            seen.add(len(a))
            assert is_sorted(a) and is_sorted(b)
            no_sentinel([a, b])
            M.check_two_way(width, content, a, b)
            assert np.array_equal(exp, orc.merge(a, b)), (n, sp)
            assert np.array_equal(exp, M.loop_merge([a, b], width)), (n, sp)
        assert seen == {0, n, 1, n - 1, n // 2}


@pytest.mark.parametrize("name", list(M.KWAY))
@pytest.mark.parametrize("width", WIDTHS)
def test_kway_cases(oracles, width, name):
    runs, promise = M.kway_inputs(width, name)
    assert all(is_sorted(r) for r in runs), name
    no_sentinel(runs)
    dec = M.check_promise(width, name, runs, promise)
    assert dec["k"] == len(runs)
    exp = M.kway_expected(width, name)
    assert len(exp) == sum(len(r) for r in runs)
    assert np.array_equal(exp, oracles[width].multiway_merge(runs)), name
    if name not in M.LARGE:
        assert np.array_equal(exp, M.loop_merge(runs, width)), name


@pytest.mark.parametrize("width", WIDTHS)
def test_kway_table_covers_the_decision(width):
    """Every form, D = 0 and D > 0, s = 0 with L < D, the largest L of the
    width, no queue, one and several queued buckets, k at both ends of the
    one-pass range and on both sides of it."""
    decs = {name: M.check_promise(width, name, *M.kway_inputs(width, name)) for name in M.KWAY}
    assert {d["form"] for d in decs.values()} == {"none", "buckets", "tree"}
    b = [d for d in decs.values() if d["form"] == "buckets"]
    assert {3, M.KM_KMAX} <= {d["k"] for d in b}
    assert {1, 2, M.KM_KMAX + 1} <= {d["k"] for d in decs.values() if d["form"] == "tree"}
    assert any(d["D"] == 0 and d["L"] == 4 * width for d in b)
    assert any(d["D"] > 0 and d["L"] == 4 * width for d in b)
    assert any(d["L"] < d["D"] and d["s"] == 0 for d in b)
    assert {0, 1, 2, 16} <= {len(d["queued"]) for d in b}
    C = M.cap(width)
    sizes = {x for d in b for x in d["sizes"]}
    assert {C // 2, C // 2 + 1, C, C + 1} <= sizes
    assert any(x > 1 << 21 for x in sizes)


@pytest.mark.parametrize("name", list(M.COUNTS))
@pytest.mark.parametrize("width", WIDTHS)
def test_count_cases(oracles, width, name):
    r, s, exp = M.count_inputs(width, name)
    assert is_sorted(r) and is_sorted(s)
    assert isinstance(exp, int) and exp == M.COUNT_PROMISE[name]
    assert exp == oracles[width].merge_join(r, s)
    if name not in M.COUNT_LARGE:
        assert exp == M.loop_count(r, s)
    lo, hi = M.limits(width)
    if name == "one_key":
        assert exp > 1 << 32 and len(np.unique(s["key"])) == 1
    if name == "stride":
        assert len(s) > M.MJ_GRID and len(np.unique(s["key"])) == len(s)
        assert np.isin(s["key"][M.MJ_GRID:], r["key"]).sum() >= 99
    if name == "end_keys":
        assert set(r["key"].tolist()) == set(s["key"].tolist()) == {lo, hi}
    if name.startswith("empty"):
        assert (len(r) == 0) != (len(s) == 0)
