"""The grouped aggregation on CPU: both libraries export
smj_dev_group_aggregate, smj_dev_group_count and smj_group_tile, and the
binding carries them up to Library.dev_group_aggregate / dev_group_count /
group_tile / group_by.  No device call is made (tests/
test_gpu_group_aggregate.py runs them; smj_group_tile is a host call).  The
expected-value construction of the GPU tests (group_ref.numpy_groups) is
checked here against the plain definition, and the cases of the GPU test are
checked to hold what their descriptions promise: conditions on the inputs,
not on the code under test."""
import ctypes
import os

import numpy as np
import pytest

import group_ref as G

NAMES = ("smj_dev_group_aggregate", "smj_dev_group_count", "smj_group_tile")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def smj_mod():
    import smj
    for w in (8, 16):
        if not os.path.exists(smj.lib_path(w)):
            smj.build()
            break
    return smj


@pytest.mark.parametrize("width", [8, 16])
def test_libraries_export_group_aggregate(smj_mod, width):
    lib = ctypes.CDLL(smj_mod.lib_path(width))
    for name in NAMES:
        assert hasattr(lib, name), name


def test_names_are_listed(smj_mod):
    for name in NAMES:
        assert name in smj_mod.DEVICE_SYMBOLS


@pytest.mark.parametrize("width", [8, 16])
def test_binding_has_group_aggregate(smj_mod, width):
    L = smj_mod.Library(width)
    # (ws, sorted, n, group_shift, key, start, count, sum, min, max, out_cap, stream)
    f = L.lib.smj_dev_group_aggregate
    assert f.restype is ctypes.c_uint64
    assert len(f.argtypes) == 12
    assert f.argtypes[2] is ctypes.c_uint64 and f.argtypes[3] is ctypes.c_uint32
    assert f.argtypes[10] is ctypes.c_uint64
    # (ws, sorted, n, group_shift, groups, stream)
    f = L.lib.smj_dev_group_count
    assert f.restype is None and len(f.argtypes) == 6 and f.argtypes[3] is ctypes.c_uint32
    assert L.lib.smj_group_tile.restype is ctypes.c_uint32
    for method in ("dev_group_aggregate", "dev_group_count", "group_tile", "group_by"):
        assert callable(getattr(L, method)), method


@pytest.mark.parametrize("width", [8, 16])
def test_tile_is_the_kernels(smj_mod, width):
    assert smj_mod.Library(width).group_tile() == G.T
    assert (G.B + 2) * G.T + 3 < 1 << 23


# key domains: around zero, within 40 of either end of int64, and both ends
# mixed
DOMAINS = {"mid": (-20, 20), "top": (I64_MAX - 40, I64_MAX), "bottom": (I64_MIN, I64_MIN + 40),
           "both": None}


def domain_tuples(domain, n, rng):
    t = np.zeros(n, np.dtype([("payload", "<i8"), ("key", "<i8")]))
    if domain != "both":
        a, b = DOMAINS[domain]
        t["key"] = rng.integers(a, b, n, dtype=np.int64, endpoint=True)
    else:
        off = rng.integers(0, 40, n, dtype=np.int64, endpoint=True)
        t["key"] = np.where(rng.integers(0, 2, n) == 1, I64_MAX - off, I64_MIN + off)
    # payloads at the ends of int64 among small ones: the sums wrap
    t["payload"] = rng.choice(np.array([I64_MIN, I64_MAX, I64_MAX - 1, -7, 0, 5, 1 << 62],
                                       np.int64), n)
    return G.by_key(t)


@pytest.mark.parametrize("domain", list(DOMAINS))
@pytest.mark.parametrize("shift", [0, 3, 63])
def test_numpy_construction_against_plain_loop(shift, domain):
    t = domain_tuples(domain, 300, np.random.default_rng(5))
    got, exp = G.numpy_groups(t, shift), G.loop_groups(t, shift)
    for c in G.COLUMNS:
        assert got[c].dtype == exp[c].dtype and np.array_equal(got[c], exp[c]), c
    # some sum left int64 on the way (it is kept modulo 2^64)
    true = [sum(int(p) for p in t["payload"][s:s + k]) for s, k in zip(got["start"], got["count"])]
    assert any(not I64_MIN <= s <= I64_MAX for s in true)
    assert got["count"].sum() == len(t)
    if shift == 63:
        assert len(got["key"]) == (2 if domain in ("mid", "both") else 1)
    if shift == 0:
        assert np.array_equal(got["key"], np.unique(t["key"]))


def test_run_length_form_and_empty():
    t = np.zeros(4, np.dtype([("payload", "<i4"), ("key", "<i4")]))
    t["key"], t["payload"] = [1, 1, 2, 1], [4, -9, 3, 8]
    for f in (G.numpy_groups, G.loop_groups):
        g = f(t)
        assert g["key"].tolist() == [1, 2, 1] and g["start"].tolist() == [0, 2, 3]
        assert g["count"].tolist() == [2, 1, 1] and g["sum"].tolist() == [-5, 3, 8]
        assert g["min"].tolist() == [-9, 3, 8] and g["max"].tolist() == [4, 3, 8]
        assert g["min"].dtype == np.int32 and g["sum"].dtype == np.int64
        assert all(len(v) == 0 for v in f(t[:0]).values())


def tiles_of(start, count):
    """(first tile, last tile) of every run."""
    return start // G.T, (start + count - 1) // G.T


@pytest.mark.parametrize("width", [8, 16])
def test_cases_hold_what_they_promise(width):
    lo, hi = G.limits(width)
    exp = {name: G.expected(width, name) for name in G.CASES}
    rel = {name: G.inputs(width, name)[0] for name in G.CASES}
    shift = {name: G.inputs(width, name)[1] for name in G.CASES}
    groups = {name: len(exp[name]["key"]) for name in G.CASES}
    for name in G.CASES:   # every case: a relation of this width, its runs cover it
        assert rel[name].dtype.itemsize == width
        assert exp[name]["count"].sum() == len(rel[name])
        if name != "run_length":
            assert (np.diff(rel[name]["key"].astype(np.int64)) >= 0).all(), name
    # the sizes: short runs, the last group ends in a partial (or exactly full) tile
    for name, n in G.SIZES.items():
        assert len(rel[name]) == n and shift[name] == 0
        if n > 1:
            assert n / 6 < groups[name] < n / 1.5, (name, groups[name])
    # payload order: some run's minimum is not at either of its ends, and some
    # run's payloads are not monotone
    t, e = rel["n3Tp1"], exp["n3Tp1"]
    first, last = t["payload"][e["start"]], t["payload"][e["start"] + e["count"] - 1]
    assert ((e["min"] != first) & (e["min"] != last)).any()
    assert ((e["max"] != first) & (e["max"] != last)).any()
    assert any(np.any(np.diff(t["payload"][s:s + k].astype(np.int64)) > 0) and
               np.any(np.diff(t["payload"][s:s + k].astype(np.int64)) < 0)
               for s, k in zip(e["start"], e["count"]) if k >= 3)
    # all distinct: the output is as long as the input
    assert groups["all_distinct"] == len(rel["all_distinct"]) == 2 * G.T + 5
    # one key: one group over six tiles (B + 3 tiles: more than one workgroup of
    # the carry step), the extremes in middle tiles
    for name, tiles in (("one_key_short", 6), ("one_key_long", G.B + 3)):
        t, e = rel[name], exp[name]
        assert groups[name] == 1 and -(-len(t) // G.T) == tiles
        for pos in (int(np.argmin(t["payload"])), int(np.argmax(t["payload"]))):
            assert 0 < pos // G.T < tiles - 1, (name, pos)
    assert len(rel["one_key_long"]) == (G.B + 2) * G.T + 3 < 1 << 23
    # boundaries
    e = exp["end_at_tile"]
    ends = e["start"] + e["count"] - 1
    assert G.T - 1 in ends and G.T in e["start"]
    e = exp["head_last_of_tile"]
    i = e["start"].tolist().index(G.T - 1)
    assert e["count"][i] > 1
    e = exp["mid0_to_mid3"]
    assert e["start"][1] == G.T // 2 and e["start"][1] + e["count"][1] == 3 * G.T + G.T // 2
    assert (e["count"][2:] == 1).all() and len(e["count"]) > G.T // 2
    ft, lt = tiles_of(e["start"], e["count"])
    assert (ft[1], lt[1]) == (0, 3)
    # extremes: keys at both ends; the sum of the largest payload repeated
    # leaves the payload type (and wraps at 16 bytes); negative payloads
    t, e = rel["extremes"], exp["extremes"]
    assert t["key"].min() == lo and t["key"].max() == hi
    assert e["min"][0] == e["max"][0] == hi and e["count"][0] == 5
    wrapped = (5 * hi + (1 << 63)) % (1 << 64) - (1 << 63)
    assert int(e["sum"][0]) == wrapped and (wrapped != 5 * hi) == (width == 16)
    assert not lo <= 5 * hi <= hi
    assert e["min"][2] == e["max"][2] == lo
    assert e["max"][3] < 0
    assert e["min"][5] == lo and e["max"][5] == hi
    ft, lt = tiles_of(e["start"], e["count"])
    assert (lt > ft).sum() >= 2
    # group shifts: negative and non-negative keys; at 63 the two signs
    for name in ("shift3", "shift63"):
        t = rel[name]
        assert t["key"].min() == lo and t["key"].max() == hi and shift[name] == int(name[5:])
    assert groups["shift63"] == 2
    assert exp["shift63"]["count"].tolist() == [int((rel["shift63"]["key"] < 0).sum()),
                                                int((rel["shift63"]["key"] >= 0).sum())]
    assert groups["shift3"] < len(np.unique(rel["shift3"]["key"]))
    assert set((exp["shift3"]["key"].astype(np.int64) >> 3).tolist()) >= set(range(-38, 37))
    # long groups: the first key of a group is not its last, runs cross tiles
    t, e = rel["long_groups"], exp["long_groups"]
    assert shift["long_groups"] == 12 and 8 <= groups["long_groups"] <= 11
    assert (t["key"][e["start"] + e["count"] - 1] != e["key"]).all()
    ft, lt = tiles_of(e["start"], e["count"])
    assert (lt > ft).sum() >= 3
    # run-length semantics
    assert rel["run_length"]["key"].tolist() == [1, 1, 2, 1] and groups["run_length"] == 3
