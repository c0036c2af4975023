"""The window functions on CPU: both libraries export smj_dev_window and
smj_window_tile, and the binding carries them up to Library.dev_window /
window_tile / window.  No device call is made (tests/test_gpu_window.py runs
them; smj_window_tile is a host call).  The expected-value construction of the
GPU tests (window_ref.numpy_window) is checked here against the plain
definition and against group_ref.numpy_groups, and the new cases of the GPU
test are checked to hold what their descriptions promise: conditions on the
inputs, not on the code under test."""
import ctypes
import os

import numpy as np
import pytest

import group_ref as G
import window_ref as W
from test_group_aggregate_abi import DOMAINS, I64_MAX, I64_MIN, domain_tuples

NAMES = ("smj_dev_window", "smj_window_tile")


@pytest.fixture(scope="module")
def smj_mod():
    import smj
    for w in (8, 16):
        if not os.path.exists(smj.lib_path(w)):
            smj.build()
            break
    return smj


@pytest.mark.parametrize("width", [8, 16])
def test_libraries_export_window(smj_mod, width):
    lib = ctypes.CDLL(smj_mod.lib_path(width))
    for name in NAMES:
        assert hasattr(lib, name), name


def test_names_are_listed(smj_mod):
    for name in NAMES:
        assert name in smj_mod.DEVICE_SYMBOLS


@pytest.mark.parametrize("width", [8, 16])
def test_binding_has_window(smj_mod, width):
    L = smj_mod.Library(width)
    # (ws, sorted, n, group_shift, group, row, rank, dense_rank, sum, min, max, stream)
    f = L.lib.smj_dev_window
    assert f.restype is None
    assert len(f.argtypes) == 12
    assert f.argtypes[2] is ctypes.c_uint64 and f.argtypes[3] is ctypes.c_uint32
    assert L.lib.smj_window_tile.restype is ctypes.c_uint32
    for method in ("dev_window", "window_tile", "window"):
        assert callable(getattr(L, method)), method


@pytest.mark.parametrize("width", [8, 16])
def test_tile_is_the_kernels(smj_mod, width):
    assert smj_mod.Library(width).window_tile() == W.T
    assert (W.T, W.B) == (G.T, G.B)
    assert (W.B + 2) * W.T + 3 < 1 << 23


def test_group_shift_is_checked(smj_mod):
    L = smj_mod.Library(16)
    assert L._group_shift(63) == 63
    with pytest.raises(AssertionError):
        L._group_shift(64)


@pytest.mark.parametrize("domain", list(DOMAINS))
@pytest.mark.parametrize("shift", [0, 3, 63])
def test_numpy_construction_against_plain_loop(shift, domain):
    t = domain_tuples(domain, 300, np.random.default_rng(5))
    got, exp = W.numpy_window(t, shift), W.loop_window(t, shift)
    for c in W.COLUMNS:
        assert got[c].dtype == exp[c].dtype and np.array_equal(got[c], exp[c]), c
    # some running sum left int64 on the way (it is kept modulo 2^64)
    head, _ = W.heads(t, shift)
    true, run = [], 0
    for i in range(len(t)):
        run = int(t["payload"][i]) + (0 if head[i] else run)
        true.append(run)
    assert any(not I64_MIN <= s <= I64_MAX for s in true)
    if shift == 0:
        assert not got["rank"].any() and not got["dense_rank"].any() and got["row"].any()
    if shift == 63:
        assert got["group"][-1] == (1 if domain in ("mid", "both") else 0)


def test_run_length_form_and_empty():
    t = np.zeros(4, np.dtype([("payload", "<i4"), ("key", "<i4")]))
    t["key"], t["payload"] = [1, 1, 2, 1], [4, -9, 3, 8]
    for f in (W.numpy_window, W.loop_window):
        g = f(t)
        assert g["group"].tolist() == [0, 0, 1, 2] and g["row"].tolist() == [0, 1, 0, 0]
        assert g["rank"].tolist() == [0] * 4 and g["dense_rank"].tolist() == [0] * 4
        assert g["sum"].tolist() == [4, -5, 3, 8]
        assert g["min"].tolist() == [4, -9, 3, 8] and g["max"].tolist() == [4, 4, 3, 8]
        assert g["min"].dtype == np.int32 and g["sum"].dtype == np.int64
        g = f(t, 2)   # one group 0 of the keys 1, 1, 2, 1
        assert g["group"].tolist() == [0] * 4 and g["row"].tolist() == [0, 1, 2, 3]
        assert g["rank"].tolist() == [0, 0, 2, 3] and g["dense_rank"].tolist() == [0, 0, 1, 2]
        assert all(len(v) == 0 for v in f(t[:0]).values())
        assert [v.dtype for v in f(t[:0]).values()] == [np.int64] * 5 + [np.int32] * 2


@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("name", list(W.CASES))
def test_identities_of_the_reference(width, name):
    """What ties the columns to each other and to the group table."""
    t, shift = W.inputs(width, name)
    w, g = W.expected(width, name), G.numpy_groups(t, shift)
    n, groups = len(t), len(g["key"])
    assert all(len(w[c]) == n for c in W.COLUMNS)
    assert np.array_equal(w["group"], np.repeat(np.arange(groups), g["count"]))
    assert np.array_equal(g["start"][w["group"]] + w["row"], np.arange(n))
    assert (w["rank"] <= w["row"]).all() and (w["dense_rank"] <= w["rank"]).all()
    assert (w["dense_rank"] >= 0).all()
    last = g["start"] + g["count"] - 1
    for c in ("sum", "min", "max"):
        assert w[c].dtype == g[c].dtype and np.array_equal(w[c][last], g[c]), c
    assert np.array_equal(w["row"][last] + 1, g["count"])
    if shift == 0:
        assert not w["rank"].any() and not w["dense_rank"].any()


@pytest.mark.parametrize("width", [8, 16])
def test_new_cases_hold_what_they_promise(width):
    T, B = W.T, W.B
    rel = {name: W.inputs(width, name)[0] for name in W.NEW}
    shift = {name: W.inputs(width, name)[1] for name in W.NEW}
    exp = {name: W.expected(width, name) for name in W.NEW}
    hk = {name: W.heads(rel[name], shift[name]) for name in W.NEW}
    assert set(W.CASES) == set(G.CASES) | set(W.NEW) and len(W.NEW) == 5
    for name in W.NEW:
        assert rel[name].dtype.itemsize == width
        assert (np.diff(rel[name]["key"].astype(np.int64)) >= 0).all(), name
        assert len(rel[name]) <= (B + 2) * T + 3 < 1 << 23
    # peers: a key run from the middle of tile 0 to the middle of tile 2 in a
    # group that began earlier in tile 0, so over all of tile 1 both heads lie
    # in front of the tile, and of every chunk of it
    e, (head, khead) = exp["peers_cross_tiles"], hk["peers_cross_tiles"]
    assert shift["peers_cross_tiles"] == 8
    i = np.arange(T, 2 * T)
    h, p = i - e["row"][i], i - e["row"][i] + e["rank"][i]
    assert len(set(h)) == 1 and len(set(p)) == 1 and 0 < h[0] < p[0] < T
    assert T // 4 < p[0] < 3 * T // 4
    end = int(p[0] + np.flatnonzero(khead[p[0] + 1:])[0])   # the run's last element
    assert 2 * T + T // 4 < end < 2 * T + 3 * T // 4 and not head[end + 1]
    assert e["dense_rank"][T] == 1 and e["dense_rank"][end + 1] == 2
    # tile edges: key-only heads at T - 1 and T, a group head at 2 T
    (head, khead) = hk["key_head_at_tile_edges"]
    assert shift["key_head_at_tile_edges"] == 8
    for pos in (T - 1, T):
        assert khead[pos] and not head[pos]
    assert head[2 * T] and np.flatnonzero(head).tolist() == [0, 2 * T]
    # dense_far: one group over B + 3 tiles in key runs of about 3; dense_rank
    # reaches about n / 3 and rank follows it
    t, e = rel["dense_far"], exp["dense_far"]
    n = len(t)
    assert n == (B + 2) * T + 3 and shift["dense_far"] == 20 and e["group"][-1] == 0
    assert n / 3.5 < e["dense_rank"][-1] + 1 < n / 2.5
    assert e["rank"][-1] > n - 50 and (e["rank"] <= e["row"]).all()
    assert e["dense_rank"][(B + 1) * T] > B * T / 3.5   # far behind the first carry workgroup
    # dense_resets: the far group ends in the middle of a tile behind the
    # first carry workgroup; 40 groups of three keys follow, ranks from 0 again
    t, e, (head, khead) = rel["dense_resets"], exp["dense_resets"], hk["dense_resets"]
    starts = np.flatnonzero(head)
    assert shift["dense_resets"] == 20 and len(starts) == 41
    assert starts[1] // T == B + 1 and T // 4 < starts[1] % T < 3 * T // 4
    assert e["dense_rank"][starts[1] - 1] > starts[1] / 3.5
    assert not e["dense_rank"][starts].any() and not e["rank"][starts].any()
    for s in starts[1:]:
        assert e["dense_rank"][s:s + 6].tolist() == [0, 0, 1, 2, 2, 2]
        assert e["rank"][s:s + 6].tolist() == [0, 0, 2, 3, 3, 3]
    # shift0_ranks: repeated keys, no group shift
    e = exp["shift0_ranks"]
    assert shift["shift0_ranks"] == 0 and len(rel["shift0_ranks"]) > 2 * T
    assert not e["rank"].any() and not e["dense_rank"].any() and e["row"].max() >= 3
    # the imported cases the issue names
    assert len(W.inputs(width, "n1")[0]) == 1
    assert W.inputs(width, "run_length")[0]["key"].tolist() == [1, 1, 2, 1]
