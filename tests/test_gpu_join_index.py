"""Join index and semi/anti joins (smj_dev_join_pairs, smj_dev_semi_join).

Expected values come from an independent numpy construction over the sorted
relations (numpy_pairs, numpy_semi_mask): per key of S, the R run and the S
run, the output R-major -- for each R tuple of the run, the whole S run.  The
inputs are sorted by the oracle, so 8-byte ties follow the packed-word order.
Every comparison is bit-exact, at both widths.

Sizes are the smallest that reach each path of the kernels: tiles are 512 S
elements, the R window staged in LDS holds 1024 keys, a work item is 8192
outputs.
"""
import numpy as np
import pytest

from test_gpu_parity import rand_tuples

pytestmark = pytest.mark.gpu

SENTINEL = -77


def numpy_pairs(R, S):
    """(r_idx, s_idx) into sorted R, S per output position."""
    if len(R) == 0 or len(S) == 0:
        z = np.zeros(0, np.int64)
        return z, z
    keys, s0, sc = np.unique(S["key"], return_index=True, return_counts=True)
    rlo = np.searchsorted(R["key"], keys, "left")
    rc = np.searchsorted(R["key"], keys, "right") - rlo
    per = rc * sc
    run = np.repeat(np.arange(len(keys)), per)
    pos = np.arange(per.sum()) - np.concatenate([[0], np.cumsum(per)[:-1]])[run]
    return rlo[run] + pos // sc[run], s0[run] + pos % sc[run]


def numpy_semi_mask(R, S):
    return np.searchsorted(R["key"], S["key"], "right") > \
        np.searchsorted(R["key"], S["key"], "left")


def with_keys(t, keys):
    t["key"] = keys
    return t


def case_keyjoin(width):
    """R unique keys 1..3000; S 1300 tuples (a ragged last tile) over keys
    1..4000, so some have no partner: bitmap tiles with the partner gather."""
    rng = np.random.default_rng(21)
    R = with_keys(rand_tuples(width, 3000, 1), rng.permutation(3000) + 1)
    S = rand_tuples(width, 1300, 2, 1, 4001)
    return R, S


def case_dups(width):
    """Duplicates on both sides, negative keys: multi tiles, S runs that
    straddle tile boundaries."""
    return rand_tuples(width, 3000, 5, -200, 200), rand_tuples(width, 4000, 6, -200, 220)


def case_hot(width):
    """600 R and 1500 S tuples share key 777: one run of 900 000 pairs (more
    than 100 work items), its S run across 3+ tiles; 100 S tuples have a key
    absent from R."""
    R = rand_tuples(width, 2000, 11, 0, 2000)
    S = rand_tuples(width, 3000, 12, 0, 2000)
    R["key"][:600] = 777
    S["key"][:1500] = 777
    S["key"][1500:1600] = 5000
    return R, S


def case_unstaged(width):
    """3 distinct keys in 5000 R tuples: the one S tile's R window exceeds
    the 1024 staged keys (the global-memory search)."""
    rng = np.random.default_rng(31)
    R = with_keys(rand_tuples(width, 5000, 13), rng.choice([10, 20, 30], 5000))
    S = with_keys(rand_tuples(width, 600, 14), rng.choice([10, 20, 30, 40], 600))
    return R, S


def case_mixed(width):
    """A key-join key range next to a duplicate-heavy one: bitmap tiles and
    multi tiles as neighbours in one call."""
    Ra, Sa = case_keyjoin(width)
    Rb = rand_tuples(width, 3000, 15, 10000, 10400)
    Sb = rand_tuples(width, 4000, 16, 10000, 10420)
    return np.concatenate([Ra, Rb]), np.concatenate([Sa, Sb])


def tiny(nr, ns, s_extra=1):
    """keys 5..7 in R; in S also 8 (s_extra), which has no partner"""
    def make(width):
        return rand_tuples(width, nr, 3, 5, 8), rand_tuples(width, ns, 4, 5, 8 + s_extra)
    return make


def case_one_one(width):
    return rand_tuples(width, 1, 3, 7, 8), rand_tuples(width, 1, 4, 7, 8)  # both key 7


CASES = {
    "empty_R": tiny(0, 5), "empty_S": tiny(5, 0), "one_one": case_one_one,
    "tiny_700": tiny(3, 700), "keyjoin": case_keyjoin, "dups": case_dups,
    "hot": case_hot, "unstaged": case_unstaged, "mixed": case_mixed,
}
_prepared = {}


def prepared(orc, width, name):
    """Sorted inputs and the expected index of a case, computed once."""
    if (width, name) not in _prepared:
        R, S = CASES[name](width)
        R, S = orc.sort(R), orc.sort(S)
        for a in (R, S):
            a.setflags(write=False)
        _prepared[width, name] = (R, S) + numpy_pairs(R, S)
    return _prepared[width, name]


def filled(dtype, n):
    a = np.zeros(n, dtype)
    a["key"] = a["payload"] = SENTINEL
    return a


def column(lib, n, fill=SENTINEL):
    import torch
    return torch.full((n,), fill, dtype=torch.int32 if lib.width == 8 else torch.int64,
                      device="cuda")


def run_pairs(lib, dR, dS, cap, room=5, keys=True):
    """dev_join_pairs into the first `cap` elements of columns with `room`
    more; the elements past the capacity must keep their fill."""
    import torch
    bufs = [column(lib, cap + room) for _ in range(3 if keys else 2)]
    total = lib.dev_join_pairs(dR, dS, *[b[:cap] for b in bufs])
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for h in host:
        assert np.all(h[cap:] == SENTINEL)
    return total, [h[:cap] for h in host]


def check_pairs(cols, R, S, r_idx, s_idx):
    """The first len(cols[0]) outputs of dev_join_pairs: the R payloads, the
    S payloads and, with a third column, the keys (of either side)."""
    n = len(cols[0])
    assert np.array_equal(cols[0], R["payload"][r_idx[:n]])
    assert np.array_equal(cols[1], S["payload"][s_idx[:n]])
    if len(cols) == 3:
        assert np.array_equal(cols[2], S["key"][s_idx[:n]])
        assert np.array_equal(cols[2], R["key"][r_idx[:n]])


def test_numpy_construction_against_double_loop():
    """The expected-value construction itself, against the plain definition."""
    R = np.sort(rand_tuples(16, 40, 1, 0, 12), order=["key", "payload"])
    S = np.sort(rand_tuples(16, 60, 2, 0, 14), order=["key", "payload"])
    exp = [(i, j) for k in np.unique(S["key"])
           for i in np.flatnonzero(R["key"] == k) for j in np.flatnonzero(S["key"] == k)]
    r_idx, s_idx = numpy_pairs(R, S)
    assert exp == list(zip(r_idx.tolist(), s_idx.tolist()))
    assert np.array_equal(numpy_semi_mask(R, S), np.isin(S["key"], R["key"]))


@pytest.mark.parametrize("name", list(CASES))
def test_pairs_and_semi(libs, oracles, width, name):
    import torch
    orc, lib = oracles[width], libs[width]
    R, S, r_idx, s_idx = prepared(orc, width, name)
    total = len(r_idx)
    assert total == orc.merge_join(R, S)
    dR, dS = lib.to_device(R), lib.to_device(S)
    assert lib.dev_join_pairs(dR, dS) == total  # count only
    got, (r, s, k) = run_pairs(lib, dR, dS, total)
    assert got == total
    check_pairs((r, s, k), R, S, r_idx, s_idx)
    # without the key column
    got, (r2, s2) = run_pairs(lib, dR, dS, total, keys=False)
    assert got == total and np.array_equal(r2, r) and np.array_equal(s2, s)
    # the order is the materialised output's
    mat = lib.empty(total)
    assert lib.dev_materialize(dR, dS, mat) == total
    torch.cuda.synchronize()
    mat = lib.to_host(mat)
    assert np.array_equal(s, mat["payload"]) and np.array_equal(k, mat["key"])
    # semi and anti joins of S
    mask = numpy_semi_mask(R, S) if len(R) else np.zeros(len(S), bool)
    outs = []
    for anti, m in ((False, mask), (True, ~mask)):
        n = int(m.sum())
        assert lib.dev_semi_join(dR, dS, anti=anti) == n  # count only
        out = lib.to_device(filled(S.dtype, n + 3))
        assert lib.dev_semi_join(dR, dS, out[:n], anti=anti) == n
        torch.cuda.synchronize()
        out = lib.to_host(out)
        assert np.array_equal(out[:n], S[m])
        assert np.all(out[n:]["key"] == SENTINEL) and np.all(out[n:]["payload"] == SENTINEL)
        outs.append(out[:n])
    assert len(outs[0]) + len(outs[1]) == len(S)
    if name == "empty_R":
        assert len(outs[0]) == 0 and np.array_equal(outs[1], S)
    assert np.array_equal(orc.sort(np.concatenate(outs)), S)
    # the same filter on the R side: the arguments swapped
    rmask = numpy_semi_mask(S, R) if len(S) else np.zeros(len(R), bool)
    assert lib.dev_semi_join(dS, dR) == int(rmask.sum())


def test_capacity(libs, oracles, width):
    """A short buffer receives the prefix and the total is still returned."""
    orc, lib = oracles[width], libs[width]
    R, S, r_idx, s_idx = prepared(orc, width, "hot")
    total = len(r_idx)
    assert total >= 900_000
    dR, dS = lib.to_device(R), lib.to_device(S)
    cap = total // 3 + 17
    got, (r, s, k) = run_pairs(lib, dR, dS, cap, room=20000)
    assert got == total
    check_pairs((r, s, k), R, S, r_idx, s_idx)
    assert lib.dev_join_pairs(dR, dS) == total
    # semi join into a short buffer
    mask = numpy_semi_mask(R, S)
    n = int(mask.sum())
    import torch
    out = lib.to_device(filled(S.dtype, n))
    assert lib.dev_semi_join(dR, dS, out[:n // 2]) == n
    torch.cuda.synchronize()
    out = lib.to_host(out)
    assert np.array_equal(out[:n // 2], S[mask][:n // 2])
    assert np.all(out[n // 2:]["key"] == SENTINEL)


def test_total_above_2_32(libs, oracles, width):
    """One key on both sides, 70 000 x 70 000: the total needs 64 bits."""
    orc, lib = oracles[width], libs[width]
    n = 70_000
    R = orc.sort(rand_tuples(width, n, 17, 42, 43))
    S = orc.sort(rand_tuples(width, n, 18, 42, 43))
    dR, dS = lib.to_device(R), lib.to_device(S)
    assert lib.dev_join_pairs(dR, dS) == n * n
    got, (r, s, k) = run_pairs(lib, dR, dS, 1000)
    assert got == n * n
    # R-major: the first |S| outputs pair R[0] with the S run in order
    assert np.all(r == R["payload"][0])
    assert np.array_equal(s, S["payload"][:1000])
    assert np.all(k == 42)
    assert lib.dev_semi_join(dR, dS) == n and lib.dev_semi_join(dR, dS, anti=True) == 0


ROW0 = 5  # the generators' payload is 5 + row id


def test_join_index_pk_fk(libs, width):
    """The one-call form on unsorted relations whose payloads are row ids."""
    import torch
    lib = libs[width]
    n = 1 << 16
    R, S = lib.empty(n), lib.empty(n)
    lib.dev_gen_pk(R, 0, n, 12345)
    lib.dev_gen_fk(S, 0, n, n, 54321)
    r, s, k = lib.join_index(R, S, key_range=(1, n), with_keys=True)
    r2, s2 = lib.join_index(R, S)
    torch.cuda.synchronize()
    assert torch.equal(r, r2) and torch.equal(s, s2)
    Rh, Sh, off = lib.to_host(R), lib.to_host(S), ROW0
    r, s, k = (x.cpu().numpy().astype(np.int64) for x in (r, s, k))
    assert len(r) == len(s) == len(k) == n
    assert np.array_equal(Rh["key"][r - off], k)
    assert np.array_equal(Sh["key"][s - off], k)
    assert np.all(np.diff(k) >= 0)
    assert np.array_equal(np.sort(s), np.arange(n) + off)  # every S row once


def test_join_index_zipf(libs, oracles, width):
    import torch
    orc, lib = oracles[width], libs[width]
    n = 1 << 16
    R, S = lib.empty(n), lib.empty(n)
    lib.dev_gen_pk(R, 0, n, 12345)
    lib.dev_gen_zipf(S, 0, n, 0.75, 777)
    S[:, 0] = torch.arange(ROW0, n + ROW0, device="cuda", dtype=S.dtype)  # row ids
    r, s, k = lib.join_index(R, S, with_keys=True)
    torch.cuda.synchronize()
    Rs, Ss = orc.sort(lib.to_host(R)), orc.sort(lib.to_host(S))
    r_idx, s_idx = numpy_pairs(Rs, Ss)
    assert len(r_idx) == orc.merge_join(Rs, Ss) == len(r)
    assert np.array_equal(r.cpu().numpy(), Rs["payload"][r_idx])
    assert np.array_equal(s.cpu().numpy(), Ss["payload"][s_idx])
    assert np.array_equal(k.cpu().numpy(), Ss["key"][s_idx])
