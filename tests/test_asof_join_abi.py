"""The as-of join entry point on CPU: both libraries export smj_dev_asof_join
and the binding carries it up to Library.dev_asof_join / asof_join.  No
device call is made (tests/test_gpu_asof_join.py runs them).  The
expected-value construction of the GPU tests (asof_ref.numpy_asof) is checked
here against the plain definition, and the cases of the GPU test are checked
to hold what their descriptions promise: conditions on the inputs, not on the
code under test."""
import ctypes
import os

import numpy as np
import pytest

import asof_ref as A
from band_ref import I64_MAX, I64_MIN

NAME = "smj_dev_asof_join"


@pytest.fixture(scope="module")
def smj_mod():
    import smj
    for w in (8, 16):
        if not os.path.exists(smj.lib_path(w)):
            smj.build()
            break
    return smj


@pytest.mark.parametrize("width", [8, 16])
def test_libraries_export_asof_join(smj_mod, width):
    assert hasattr(ctypes.CDLL(smj_mod.lib_path(width)), NAME)


def test_name_is_listed(smj_mod):
    assert NAME in smj_mod.DEVICE_SYMBOLS


@pytest.mark.parametrize("width", [8, 16])
def test_binding_has_asof_join(smj_mod, width):
    L = smj_mod.Library(width)
    # (ws, R, nR, S, nS, mode, tolerance, group_shift, r_index, r_payload, r_key, matched,
    #  stream)
    f = L.lib.smj_dev_asof_join
    assert f.restype is None
    assert len(f.argtypes) == 13
    assert f.argtypes[5] is ctypes.c_uint32
    assert f.argtypes[6] is ctypes.c_uint64
    assert f.argtypes[7] is ctypes.c_uint32
    for method in ("dev_asof_join", "asof_join"):
        assert callable(getattr(L, method)), method


# key domains: around zero, within 30 of either end of int64, and both ends
# mixed (a distance then needs 64 unsigned bits)
DOMAINS = {"mid": (-15, 15), "top": (I64_MAX - 30, I64_MAX), "bottom": (I64_MIN, I64_MIN + 30),
           "both": None}
TOLERANCES = [0, 3, 1 << 63, (1 << 64) - 1]


def domain_keys(domain, n, rng):
    if domain != "both":
        a, b = DOMAINS[domain]
        return np.sort(rng.integers(a, b, n, dtype=np.int64, endpoint=True))
    off = rng.integers(0, 30, n, dtype=np.int64, endpoint=True)
    return np.sort(np.where(rng.integers(0, 2, n) == 1, I64_MAX - off, I64_MIN + off))


@pytest.mark.parametrize("domain", list(DOMAINS))
@pytest.mark.parametrize("group_shift", [0, 3])
@pytest.mark.parametrize("tolerance", TOLERANCES, ids=[f"tol{i}" for i in range(len(TOLERANCES))])
@pytest.mark.parametrize("direction,strict", A.MODES)
def test_numpy_construction_against_double_loop(direction, strict, tolerance, group_shift, domain):
    rng = np.random.default_rng(7)
    Rk, Sk = domain_keys(domain, 40, rng), domain_keys(domain, 50, rng)
    got = A.numpy_asof(Rk, Sk, direction, strict, tolerance, group_shift)
    exp = A.double_loop(Rk, Sk, direction, strict, tolerance, group_shift)
    assert got.dtype == np.int64 and np.array_equal(got, exp)
    if tolerance == (1 << 64) - 1:   # UINT64_MAX is no limit
        assert np.array_equal(got, A.numpy_asof(Rk, Sk, direction, strict, None, group_shift))
    if domain == "both" and direction == "backward" and not strict and group_shift == 0:
        # some S key at the top has its B at the bottom: a distance above 2^63
        d = [int(Sk[i]) - int(Rk[p]) for i, p in enumerate(exp) if p >= 0]
        assert (max(d, default=0) > 1 << 63) == (tolerance == (1 << 64) - 1)


def test_empty_sides():
    keys = np.arange(5, dtype=np.int64)
    for f in (A.numpy_asof, A.double_loop):
        assert np.array_equal(f(keys[:0], keys), np.full(5, -1))
        assert f(keys, keys[:0]).shape == (0,)


def matched(orc, width, name, tol, gsh):
    return {m: int((A.expected(orc, width, name, *m, tol, gsh) >= 0).sum()) for m in A.MODES}


@pytest.mark.parametrize("width", [8, 16])
def test_cases_hold_what_they_promise(oracles, width):
    orc = oracles[width]
    nS = {name: len(A.inputs(orc, width, name)[1]) for name in A.CASES}
    # the cases that promise matched and unmatched rows, in every mode
    for name, tol, gsh in A.MIXED:
        assert (tol, gsh) in A.CASES[name][1](width)
        for m, k in matched(orc, width, name, tol, gsh).items():
            assert 0 < k < nS[name], (name, tol, gsh, m, k)
    # the sizes
    for name, n in (("s511", 511), ("s512", 512), ("s513", 513), ("s1025", 1025)):
        assert nS[name] == n and len(A.inputs(orc, width, name)[0]) == 3000
    assert len(A.inputs(orc, width, "empty_R")[0]) == 0 and nS["empty_R"] == 5
    assert len(A.inputs(orc, width, "empty_S")[0]) == 5 and nS["empty_S"] == 0
    assert len(A.inputs(orc, width, "one_R_many_S")[0]) == 1 and nS["one_R_many_S"] == 3000
    assert len(A.inputs(orc, width, "sparse_R")[0]) == 5 and nS["sparse_R"] == 3000
    # one_one: both keys 7; strict gives none
    R, S = A.inputs(orc, width, "one_one")
    assert R["key"].tolist() == [7] and S["key"].tolist() == [7]
    assert matched(orc, width, "one_one", None, 0) == {m: 0 if m[1] else 1 for m in A.MODES}
    # dups: some S key has >= 2 equal R keys; backward takes the last of the
    # run and forward the first
    R, S = A.inputs(orc, width, "dups")
    lb, ub = np.searchsorted(R["key"], S["key"], "left"), np.searchsorted(R["key"], S["key"], "right")
    runs = ub - lb >= 2
    assert runs.any()
    back = A.expected(orc, width, "dups", "backward", False, None, 0)
    fwd = A.expected(orc, width, "dups", "forward", False, None, 0)
    assert np.array_equal(back[runs], ub[runs] - 1) and np.array_equal(fwd[runs], lb[runs])
    assert (back[runs] > fwd[runs]).all()
    # all_below / all_above: backward (forward) takes the last (first) R tuple
    # for every row and the other direction finds none
    for name, hit, miss, pos in (("all_below", "backward", "forward", -1),
                                 ("all_above", "forward", "backward", 0)):
        R, S = A.inputs(orc, width, name)
        if pos < 0:
            assert R["key"].max() < S["key"].min()
        else:
            assert R["key"].min() > S["key"].max()
        for strict in (False, True):
            assert (A.expected(orc, width, name, hit, strict, None, 0) == pos % len(R)).all()
            assert (A.expected(orc, width, name, miss, strict, None, 0) == -1).all()
    # wide: windows beyond the staged 1024 keys; every other case but it fits
    R, S = A.inputs(orc, width, "wide")
    assert min(A.tile_windows(R["key"], S["key"])) > A.RWIN
    R, S = A.inputs(orc, width, "dups")
    assert max(A.tile_windows(R["key"], S["key"])) <= A.RWIN
    # groups: R lacks two of S's groups, some are negative, and some S row's
    # ungrouped B lies in another group: the row comes out unmatched
    # (backward) or takes its F (nearest)
    R, S = A.inputs(orc, width, "groups")
    gR, gS = set((R["key"] >> A.GROUP_SHIFT).tolist()), set((S["key"] >> A.GROUP_SHIFT).tolist())
    assert gS == set(A.S_GROUPS) and gR == set(A.R_GROUPS) and len(gS - gR) == 2 and min(gS) < 0
    plain = A.expected(orc, width, "groups", "backward", False, None, 0)
    other = (plain >= 0) & ((R["key"][plain] >> A.GROUP_SHIFT) != (S["key"] >> A.GROUP_SHIFT))
    assert other.any()
    grouped = A.expected(orc, width, "groups", "backward", False, None, A.GROUP_SHIFT)
    near = A.expected(orc, width, "groups", "nearest", False, None, A.GROUP_SHIFT)
    fwd = A.expected(orc, width, "groups", "forward", False, None, A.GROUP_SHIFT)
    assert (grouped[other] == -1).all() and np.array_equal(near[other], fwd[other])
    assert (near[other] >= 0).any() and (near[other] == -1).any()
    # ends: keys at both ends of the key type, the ends included; 16-byte
    # tuples: a distance above 2^63, which the tolerance 2^63 + 7 turns away
    R, S = A.inputs(orc, width, "ends")
    kmin, kmax = (I64_MIN, I64_MAX) if width == 16 else (-(1 << 31), (1 << 31) - 1)
    for t in (R, S):
        assert t["key"].min() == kmin and t["key"].max() == kmax
        assert ((t["key"] >= kmax - 50) | (t["key"] <= kmin + 50)).all()
    # (every key value occurs on both sides, so the far partners are the strict
    # ones: the B of the lowest key at the top lies at the bottom)
    for direction in ("backward", "forward"):
        far = A.expected(orc, width, "ends", direction, True, None, 0)
        dist = [abs(int(s) - int(R["key"][p])) for s, p in zip(S["key"], far) if p >= 0]
        assert max(dist) > (1 << (63 if width == 16 else 31))
        if width == 16:
            limited = A.expected(orc, width, "ends", direction, True, (1 << 63) + 7, 0)
            assert 0 < (limited >= 0).sum() < (far >= 0).sum()
        for tol in (40, 0):   # 0: a strict partner is never at distance 0
            k = (A.expected(orc, width, "ends", direction, True, tol, 0) >= 0).sum()
            assert (0 < k < (far >= 0).sum()) if tol else k == 0
