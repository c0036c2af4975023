"""Band join (smj_dev_band_join, smj_dev_band_join_count).

Expected values come from band_ref.numpy_band over the sorted relations: per
S tuple the R range of its band, S-major.  The inputs are sorted by the
oracle, so 8-byte ties follow the packed-word order.  Every comparison is
bit-exact, at both widths.  Every call writes into columns with sentinel
room behind the capacity, and the inputs are compared unchanged after it.

Sizes are the smallest that reach each path of the kernels: tiles are 512 S
elements, the R window staged in LDS holds 1024 keys, a work item is 8192
outputs.
"""
import numpy as np
import pytest

from band_ref import I64_MAX, I64_MIN, numpy_band
from test_gpu_parity import rand_tuples

pytestmark = pytest.mark.gpu

SENTINEL = -77
ROW0 = 5  # the generators' payload is 5 + row id


def with_keys(t, keys):
    t["key"] = keys
    return t


def tiny(nr, ns):
    def make(width):
        return rand_tuples(width, nr, 3, 5, 8), rand_tuples(width, ns, 4, 5, 9)
    return make


def case_one_one(width):
    return rand_tuples(width, 1, 3, 7, 8), rand_tuples(width, 1, 4, 7, 8)  # both key 7


def s_edge(ns):
    """A ragged (or exactly full) last S tile against 3000 R keys."""
    def make(width):
        return rand_tuples(width, 3000, 21, 0, 3000), rand_tuples(width, ns, 22, 0, 3000)
    return make


def case_dups(width):
    """Duplicates on both sides, negative keys: staged windows, ranges that
    overlap across tiles; about 228 000 pairs, 30 work items."""
    return rand_tuples(width, 3000, 5, -200, 200), rand_tuples(width, 4000, 6, -200, 220)


def case_one_sided(width):
    return rand_tuples(width, 3000, 31, 0, 5000), rand_tuples(width, 2000, 32, 0, 5000)


def case_wide(width):
    """Windows of about 8200 keys (searched in global memory); about 2.35M
    pairs, 290 work items, 1700 partners per S tuple."""
    return rand_tuples(width, 20000, 41, 0, 100000), rand_tuples(width, 1500, 42, 0, 100000)


def case_one_S_many_R(width):
    """One element's range over several work items, and an element with none."""
    R = with_keys(rand_tuples(width, 30000, 51), 9)
    S = with_keys(rand_tuples(width, 3, 52), np.array([9, 9, 50]))
    return R, S


def case_sparse(width):
    """Mostly empty ranges: keys below 2^40 and a band of +-2^28 (16-byte),
    the same scaled by 2^-9 into int32 (8-byte)."""
    top = 1 << 40 if width == 16 else 1 << 31
    return rand_tuples(width, 3000, 61, 0, top - 1), rand_tuples(width, 3000, 62, 0, top - 1)


def sparse_bands(width):
    d = 1 << 28 if width == 16 else 1 << 19
    return [(-d, d)]


def saturate(ends):
    """Keys within 50 of the ends of the key type (the ends included): of the
    upper end ("top"), of the lower ("bottom"), or half of each ("both")."""
    def make(width):
        kmin, kmax = (I64_MIN, I64_MAX) if width == 16 else (-(1 << 31), (1 << 31) - 1)

        def rel(n, seed):
            t = rand_tuples(width, n, seed)
            k = np.random.default_rng(seed).integers(0, 50, n)
            top = {"top": np.ones(n, bool), "bottom": np.zeros(n, bool),
                   "both": np.arange(n) % 2 == 0}[ends]
            t["key"] = np.where(top, kmax - k, kmin + k)
            t["key"][0] = kmax if top[0] else kmin
            t["key"][1] = kmax if top[1] else kmin
            return t
        return rel(700, 71), rel(600, 72)
    return make


FULL = (I64_MIN, I64_MAX)


def saturate_bands(width):
    """Sums that leave int64 (16-byte) or int32 (8-byte: lo / hi of +-2^40
    are unbounded), half-infinite bands, and narrow ones at the ends."""
    if width == 16:
        return [(1 << 62, I64_MAX), (I64_MIN, -(1 << 62)), FULL, (I64_MIN, 2), (-2, I64_MAX),
                (I64_MAX - 20, I64_MAX), (I64_MIN, I64_MIN + 20), (3, 40), (-40, -3)]
    return [(-(1 << 40), 1 << 40), (1 << 31, 1 << 40), (-(1 << 40), -(1 << 31)),
            (-(1 << 40), 2), (-2, 1 << 40), FULL, (3, 40), (-40, -3)]


def covers_all(width, name, band):
    """The bands that hold every pair: unbounded on both sides, where no
    difference of two keys leaves int64 (keys at both ends of int64 do)."""
    return name.startswith("saturate") and (width == 8 or name != "saturate") and \
        band in (FULL, (-(1 << 40), 1 << 40))


def fixed(bands):
    return lambda width: bands


# name -> (relations of a width, bands of a width)
CASES = {
    "empty_R": (tiny(0, 5), fixed([(-1, 1)])),
    "empty_S": (tiny(5, 0), fixed([(-1, 1)])),
    "one_one": (case_one_one, fixed([(0, 0), (-1, 1), (1, 2)])),
    "inverted": (case_dups, fixed([(2, 1)])),
    "s511": (s_edge(511), fixed([(-2, 2)])),
    "s512": (s_edge(512), fixed([(-2, 2)])),
    "s513": (s_edge(513), fixed([(-2, 2)])),
    "s1025": (s_edge(1025), fixed([(-2, 2)])),
    "dups": (case_dups, fixed([(-3, 4)])),
    "one_sided": (case_one_sided, fixed([(1, 6), (-7, -2)])),
    "wide": (case_wide, fixed([(-4000, 4000)])),
    "one_S_many_R": (case_one_S_many_R, fixed([(0, 0)])),
    "sparse": (case_sparse, sparse_bands),
    "saturate": (saturate("both"), saturate_bands),
    "saturate_top": (saturate("top"), saturate_bands),
    "saturate_bottom": (saturate("bottom"), saturate_bands),
}
_inputs, _expected = {}, {}


def inputs(orc, width, name):
    """Sorted inputs of a case, computed once."""
    if (width, name) not in _inputs:
        R, S = CASES[name][0](width)
        R, S = orc.sort(R), orc.sort(S)
        for a in (R, S):
            a.setflags(write=False)
        _inputs[width, name] = (R, S)
    return _inputs[width, name]


def expected(orc, width, name, band):
    """(r_idx, s_idx) of a case and band, computed once."""
    if (width, name, band) not in _expected:
        R, S = inputs(orc, width, name)
        idx = numpy_band(R["key"], S["key"], *band)
        for a in idx:
            a.setflags(write=False)
        _expected[width, name, band] = idx
    return _expected[width, name, band]


def column(lib, n, fill=SENTINEL):
    import torch
    return torch.full((n,), fill, dtype=torch.int32 if lib.width == 8 else torch.int64,
                      device="cuda")


def run_band(lib, dR, dS, band, cap, room=5, keys=True):
    """dev_band_join into the first `cap` elements of columns with `room`
    more; the elements past the capacity must keep their fill."""
    import torch
    bufs = [column(lib, cap + room) for _ in range(4 if keys else 2)]
    total = lib.dev_band_join(dR, dS, band[0], band[1], *[b[:cap] for b in bufs])
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for h in host:
        assert np.all(h[cap:] == SENTINEL)
    return total, [h[:cap] for h in host]


def check_columns(cols, R, S, r_idx, s_idx):
    n = len(cols[0])
    assert np.array_equal(cols[0], R["payload"][r_idx[:n]])
    assert np.array_equal(cols[1], S["payload"][s_idx[:n]])
    if len(cols) == 4:
        assert np.array_equal(cols[2], R["key"][r_idx[:n]])
        assert np.array_equal(cols[3], S["key"][s_idx[:n]])


def unchanged(lib, dR, dS, R, S):
    assert np.array_equal(lib.to_host(dR), R) and np.array_equal(lib.to_host(dS), S)


@pytest.mark.parametrize("name", list(CASES))
def test_band_join(libs, oracles, width, name):
    import torch
    orc, lib = oracles[width], libs[width]
    R, S = inputs(orc, width, name)
    dR, dS = lib.to_device(R), lib.to_device(S)
    for band in CASES[name][1](width):
        r_idx, s_idx = expected(orc, width, name, band)
        total = len(r_idx)
        if name == "inverted":  # 0 returned, nothing written
            assert total == 0
            got, cols = run_band(lib, dR, dS, band, 100)
            assert got == 0 and all(np.all(c == SENTINEL) for c in cols)
        if covers_all(width, name, band):
            assert total == len(R) * len(S)
        # count only: out_cap = 0, no columns
        assert lib.dev_band_join(dR, dS, *band) == total, band
        unchanged(lib, dR, dS, R, S)
        # the count form adds to the counter
        count = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        lib.dev_band_join_count(dR, dS, band[0], band[1], count)
        torch.cuda.synchronize()
        assert int(count.item()) == 5 + total, band
        unchanged(lib, dR, dS, R, S)
        # all four columns
        got, cols = run_band(lib, dR, dS, band, total)
        assert got == total, band
        check_columns(cols, R, S, r_idx, s_idx)
        unchanged(lib, dR, dS, R, S)
        if 0 < total < 300_000:  # the predicate itself, without wrap-around
            lo, hi = band
            rk, sk = cols[2].astype(object), cols[3].astype(object)
            assert np.all(sk + lo <= rk) and np.all(rk <= sk + hi)
        if name == "dups":  # both key columns NULL
            got, cols2 = run_band(lib, dR, dS, band, total, keys=False)
            assert got == total
            assert np.array_equal(cols2[0], cols[0]) and np.array_equal(cols2[1], cols[1])
            unchanged(lib, dR, dS, R, S)


def row_ids(t):
    t["payload"] = np.arange(len(t)) + ROW0
    return t


def test_equals_join_pairs_unique_R(libs, oracles, width):
    """lo = hi = 0 with R's keys unique: dev_join_pairs' columns exactly."""
    orc, lib = oracles[width], libs[width]
    rng = np.random.default_rng(21)
    R = orc.sort(with_keys(rand_tuples(width, 3000, 1), rng.permutation(3000) + 1))
    S = orc.sort(rand_tuples(width, 1300, 2, 1, 4001))
    dR, dS = lib.to_device(R), lib.to_device(S)
    total = lib.dev_join_pairs(dR, dS)
    assert total == orc.merge_join(R, S)
    pr, ps, pk = (column(lib, total) for _ in range(3))
    assert lib.dev_join_pairs(dR, dS, pr, ps, pk) == total
    got, (r, s, rk, sk) = run_band(lib, dR, dS, (0, 0), total)
    assert got == total
    assert np.array_equal(r, pr.cpu().numpy()) and np.array_equal(s, ps.cpu().numpy())
    assert np.array_equal(rk, pk.cpu().numpy()) and np.array_equal(sk, rk)


def test_equals_join_pairs_duplicates(libs, oracles, width):
    """lo = hi = 0 with duplicates on both sides: the same pairs in another
    order (payloads are distinct row ids)."""
    orc, lib = oracles[width], libs[width]
    R = orc.sort(row_ids(rand_tuples(width, 3000, 5, -200, 200)))
    S = orc.sort(row_ids(rand_tuples(width, 4000, 6, -200, 220)))
    dR, dS = lib.to_device(R), lib.to_device(S)
    total = orc.merge_join(R, S)
    pr, ps = column(lib, total), column(lib, total)
    assert lib.dev_join_pairs(dR, dS, pr, ps) == total
    got, (r, s) = run_band(lib, dR, dS, (0, 0), total, keys=False)
    assert got == total

    def as_sorted(a, b):
        p = np.stack([a.astype(np.int64), b.astype(np.int64)], axis=1)
        return p[np.lexsort((p[:, 1], p[:, 0]))]
    assert np.array_equal(as_sorted(r, s), as_sorted(pr.cpu().numpy(), ps.cpu().numpy()))


def test_capacity(libs, oracles, width):
    """A short buffer receives the exact prefix and the total is returned."""
    orc, lib = oracles[width], libs[width]
    band = (-4000, 4000)
    R, S = inputs(orc, width, "wide")
    r_idx, s_idx = expected(orc, width, "wide", band)
    total = len(r_idx)
    assert total > 2_000_000
    dR, dS = lib.to_device(R), lib.to_device(S)
    for cap in (total // 3 + 17, 1000):  # 1000: less than one work item
        got, cols = run_band(lib, dR, dS, band, cap, room=20000)
        assert got == total
        check_columns(cols, R, S, r_idx, s_idx)
    unchanged(lib, dR, dS, R, S)


def test_total_above_2_32(libs, oracles, width):
    """One key on both sides, 70 000 x 70 000: the total needs 64 bits."""
    orc, lib = oracles[width], libs[width]
    n = 70_000
    R = orc.sort(rand_tuples(width, n, 17, 42, 43))
    S = orc.sort(rand_tuples(width, n, 18, 42, 43))
    dR, dS = lib.to_device(R), lib.to_device(S)
    assert lib.dev_band_join(dR, dS, -1, 1) == n * n
    got, (r, s, rk, sk) = run_band(lib, dR, dS, (-1, 1), 1000)
    assert got == n * n
    # S-major: the first |R| outputs pair S[0] with R in order
    assert np.array_equal(r, R["payload"][:1000])
    assert np.all(s == S["payload"][0])
    assert np.all(rk == 42) and np.all(sk == 42)


def test_workspace_reuse_and_trace(libs, oracles, width):
    """wide, dups, wide on one workspace; the kernels of a call by name."""
    import torch
    orc, lib = oracles[width], libs[width]
    first = None
    for name, band in (("wide", (-4000, 4000)), ("dups", (-3, 4)), ("wide", (-4000, 4000))):
        R, S = inputs(orc, width, name)
        r_idx, s_idx = expected(orc, width, name, band)
        dR, dS = lib.to_device(R), lib.to_device(S)
        got, cols = run_band(lib, dR, dS, band, len(r_idx))
        assert got == len(r_idx)
        check_columns(cols, R, S, r_idx, s_idx)
        if name == "wide":
            if first is None:
                first = cols
            else:
                assert all(np.array_equal(a, b) for a, b in zip(first, cols))
    lib.trace(True)
    try:
        run_band(lib, dR, dS, band, len(r_idx))
        torch.cuda.synchronize()
        trace = lib.trace_read()
    finally:
        lib.trace(False)
    for k in ("k_band_bounds", "k_band_count", "k_mat_scan", "k_band_write"):
        assert trace.get(k, (0, 0))[1] == 1, (k, trace)


def test_band_join_pk_fk(libs, width):
    """The one-call form on unsorted relations whose payloads are row ids."""
    import torch
    lib = libs[width]
    n = 1 << 16
    R, S = lib.empty(n), lib.empty(n)
    lib.dev_gen_pk(R, 0, n, 12345)
    lib.dev_gen_fk(S, 0, n, n, 54321)
    Rh, Sh = lib.to_host(R), lib.to_host(S)
    r, s, rk, sk = lib.band_join(R, S, -1, 1, with_keys=True)
    r2, s2 = lib.band_join(R, S, -1, 1)
    torch.cuda.synchronize()
    assert torch.equal(r, r2) and torch.equal(s, s2)
    assert np.array_equal(lib.to_host(R), Rh) and np.array_equal(lib.to_host(S), Sh)
    r, s, rk, sk = (x.cpu().numpy().astype(np.int64) for x in (r, s, rk, sk))
    total = len(numpy_band(np.sort(Rh["key"]), np.sort(Sh["key"]), -1, 1)[0])
    assert len(r) == len(s) == len(rk) == len(sk) == total
    # the predicate, on the host copies' keys
    kr, ks = Rh["key"][r - ROW0].astype(np.int64), Sh["key"][s - ROW0].astype(np.int64)
    assert np.array_equal(kr, rk) and np.array_equal(ks, sk)
    assert np.all(ks - 1 <= kr) and np.all(kr <= ks + 1)
    assert np.all(np.diff(ks) >= 0)  # S-major: S keys never decrease
