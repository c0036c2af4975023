"""The outer join entry points on CPU: both libraries export
smj_dev_outer_join and smj_dev_outer_join_count and the binding carries them
up to Library.dev_outer_join / dev_outer_join_count / outer_join.  No device
call is made (tests/test_gpu_outer_join.py runs them).  The expected-value
construction of the GPU tests (outer_ref.numpy_outer) is checked here against
the plain definition, and the cases of the GPU test are checked to hold what
their descriptions promise: conditions on the inputs, not on the code under
test."""
import ctypes
import os

import numpy as np
import pytest

import outer_ref as O

NAMES = ("smj_dev_outer_join", "smj_dev_outer_join_count")


@pytest.fixture(scope="module")
def smj_mod():
    import smj
    for w in (8, 16):
        if not os.path.exists(smj.lib_path(w)):
            smj.build()
            break
    return smj


@pytest.mark.parametrize("width", [8, 16])
def test_libraries_export_outer_join(smj_mod, width):
    lib = ctypes.CDLL(smj_mod.lib_path(width))
    for name in NAMES:
        assert hasattr(lib, name), name


def test_names_are_listed(smj_mod):
    for name in NAMES:
        assert name in smj_mod.DEVICE_SYMBOLS
    assert smj_mod.OUTER_KEEP == O.KEEP


@pytest.mark.parametrize("width", [8, 16])
def test_binding_has_outer_join(smj_mod, width):
    L = smj_mod.Library(width)
    # (ws, R, nR, S, nS, keep, r_index, s_index, r_payload, s_payload, key, out_cap, stream)
    f = L.lib.smj_dev_outer_join
    assert f.restype is ctypes.c_uint64
    assert len(f.argtypes) == 13
    assert f.argtypes[5] is ctypes.c_uint32 and f.argtypes[11] is ctypes.c_uint64
    # (ws, R, nR, S, nS, keep, count, stream)
    g = L.lib.smj_dev_outer_join_count
    assert g.restype is None
    assert len(g.argtypes) == 8
    assert g.argtypes[5] is ctypes.c_uint32
    for method in ("dev_outer_join", "dev_outer_join_count", "outer_join"):
        assert callable(getattr(L, method)), method


class NoDevice:
    """Stands where a device tensor would: any use of it is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"touched the relation ({name}) before checking `how`")


@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("how", ["outer", "", None, "LEFT", 3])
def test_bad_how_raises_before_any_call(smj_mod, width, how):
    L = smj_mod.Library(width)
    with pytest.raises(ValueError):
        L.dev_outer_join(NoDevice(), NoDevice(), how=how)
    with pytest.raises(ValueError):
        L.dev_outer_join_count(NoDevice(), NoDevice(), how, NoDevice())
    with pytest.raises(ValueError):
        L.outer_join(NoDevice(), NoDevice(), how=how)


@pytest.mark.parametrize("seed", range(40))
def test_numpy_construction_against_double_loop(seed):
    rng = np.random.default_rng(seed)
    nR, nS = (int(x) for x in rng.integers(0, 41, 2))
    if seed % 10 == 0:
        nR = 0
    if seed % 10 == 5:
        nS = 0
    span = int(rng.integers(1, 25))
    Rk = np.sort(rng.integers(-span, span, nR, dtype=np.int64))
    Sk = np.sort(rng.integers(-span, span + 3, nS, dtype=np.int64))
    for how, keep in O.KEEP.items():
        got, exp = O.numpy_outer(Rk, Sk, keep), O.double_loop(Rk, Sk, keep)
        for g, e in zip(got, exp):
            assert g.dtype == np.int64 and np.array_equal(g, e), (how, seed)


def test_empty_sides():
    keys = np.arange(5, dtype=np.int64)
    none = keys[:0]
    for f in (O.numpy_outer, O.double_loop):
        assert all(len(c) == 0 for c in f(none, none, 3))
        r, s, k = f(none, keys, O.KEEP_S)
        assert np.all(r == -1) and np.array_equal(s, keys) and np.array_equal(k, keys)
        r, s, k = f(keys, none, O.KEEP_R)
        assert np.all(s == -1) and np.array_equal(r, keys) and np.array_equal(k, keys)
        assert len(f(none, keys, O.KEEP_R)[0]) == 0 and len(f(keys, none, O.KEEP_S)[0]) == 0


def runs(keys):
    """(start, length) of the maximal runs of equal keys"""
    starts = np.flatnonzero(np.r_[True, np.diff(keys) != 0])
    return starts, np.diff(np.r_[starts, len(keys)])


@pytest.mark.parametrize("width", [8, 16])
def test_cases_hold_what_they_promise(oracles, width):
    orc = oracles[width]
    n = {name: tuple(len(t) for t in O.inputs(orc, width, name)) for name in O.CASES}
    assert n["empty_both"] == (0, 0) and n["empty_R"] == (0, 5) and n["empty_S"] == (5, 0)
    assert n["one_one"] == n["one_lt"] == n["one_gt"] == (1, 1)
    assert n["disjoint"] == (3000, 3000) and n["keyjoin"] == (3000, 1300)
    assert n["dups"] == (3000, 4000) and n["hot"] == (2300, 3000)
    assert n["r_gaps"] == (27002, 3) and n["s_only_tiles"] == (4, 3000)
    assert n["straddle"] == (2003, 2100) and n["mixed"] == (6000, 5300)
    total = {(name, how): len(O.expected(orc, width, name, how)[0])
             for name in O.CASES for how in O.HOWS}
    # disjoint: no pairs, the full join alternates sides
    assert total["disjoint", "inner"] == 0 and total["disjoint", "full"] == 6000
    r, s, _ = O.expected(orc, width, "disjoint", "full")
    assert np.all(r[0::2] >= 0) and np.all(s[1::2] >= 0) and np.all((r < 0) != (s < 0))
    # these cases have rows of all three kinds in the full join (dups: its
    # 3000 R tuples cover all of their 401 keys, S adds keys of its own)
    assert total["dups", "full"] > total["dups", "inner"] > 0
    for name in ("keyjoin", "hot", "r_gaps", "s_only_tiles", "straddle", "mixed"):
        r, s, _ = O.expected(orc, width, name, "full")
        kinds = ((r >= 0) & (s >= 0)).any(), (s < 0).any(), (r < 0).any()
        assert all(kinds), (name, kinds)
        assert total[name, "full"] > total[name, "left"] > total[name, "inner"], name
    # keyjoin: R unique, a ragged last S tile
    R, S = O.inputs(orc, width, "keyjoin")
    assert len(np.unique(R["key"])) == len(R) and len(S) % O.TILE != 0
    # dups: negative keys, some S run crosses a tile boundary
    R, S = O.inputs(orc, width, "dups")
    st, ln = runs(S["key"])
    assert S["key"].min() < 0 and np.any(st // O.TILE != (st + ln - 1) // O.TILE)
    # hot: more than 100 work items of pairs on one key, R-only rows behind
    R, S = O.inputs(orc, width, "hot")
    assert (R["key"] == 777).sum() * (S["key"] == 777).sum() > 100 * O.PIECE
    assert (R["key"] == 6000).sum() == 300 and (S["key"] == 5000).sum() == 100
    # r_gaps: three R-only runs beyond a work item and the R window
    R, S = O.inputs(orc, width, "r_gaps")
    for k in (5, 15, 35):
        assert (R["key"] == k).sum() > max(O.PIECE, O.RWIN) and not (S["key"] == k).any()
    assert R["key"].min() < S["key"].min() and R["key"].max() > S["key"].max()
    # s_only_tiles: some whole tile of S has no partner
    R, S = O.inputs(orc, width, "s_only_tiles")
    hit = np.isin(S["key"], R["key"])
    assert any(not hit[t:t + O.TILE].any() for t in range(0, len(S), O.TILE)) and hit.sum() == 3
    # straddle: both S runs cross a tile boundary; R key 8 lies between them
    R, S = O.inputs(orc, width, "straddle")
    st, ln = runs(S["key"])
    assert len(st) == 2 and np.all(st // O.TILE != (st + ln - 1) // O.TILE)
    assert (R["key"] == 8).sum() == 2000 and (R["key"] == 9).sum() == 0
    r, s, k = O.expected(orc, width, "straddle", "full")
    assert k[np.flatnonzero(s < 0)].tolist() == [8] * 2000 and np.all(r[k == 9] == -1)
