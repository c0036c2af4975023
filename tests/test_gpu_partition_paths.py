"""Every scatter kernel of the stable partition, run and recorded.

stable_partition (csrc/partition.hip) chooses between four scatter kernels
(csrc/partition_policy.hpp; tests/test_partition_policy.py checks the choice
on the CPU).  On an MI355X every stable partition below 2^32 tuples and up to
10 digit bits takes the LDS-atomic ranks of k_scatter_swp.  The ballot ranks
with write combining (k_scatter_swc) are what a partition of 2^32 tuples, or a
device that fails smj_selfcheck_lds_order, would run; here
Library.force_ballot_ranks selects them at small sizes, and every case first
asserts with Library.last_scatter() that the kernel it is about did run.

Under the switch, up to 10 digit bits: the histogram's chunks are multiples
of 8192 tuples on at most 2048 workgroups, the scatter's tiles 4096 tuples, a
segment SEG = 8 (8-byte tuples) or 4 (16-byte) tuples, and a digit carries up
to SEG - 1 tuples from tile to tile.  Sizes and keys are chosen around those
numbers (SWC_SIZES, the key sets of make_keys).

All cases go through smj_dev_partition on the Library's workspace, the payload
is the row index (input order inside a partition is visible), and every
comparison is bit-exact: counts, offsets (64-byte aligned when padded) and
each partition's contents against the CPU oracle's partition, the steady-state
case against numpy (a stable argsort of the digits).  The output lies in an
arena of sentinels (tests/placement.py): a slot the kernel never wrote differs
from every expected tuple.
"""
import numpy as np
import pytest

from placement import arena, arena_column, check_guards

pytestmark = pytest.mark.gpu

TILE, CHUNK = 4096, 8192     # k_scatter_swc<512, 8> on the chunks of k_hist<512, 16>
# 4097: a second tile of one tuple that consumes and leaves carries; 8193: a
# second workgroup of one tuple, whose regions start anywhere modulo SEG;
# 3 * 8192 + 77: a ragged last workgroup (SEG - 1 and SEG are added per width)
SWC_SIZES = [1, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 77]
SWC_DIGITS = [(1, 0), (4, 0), (10, 0), (7, 3)]
KEYS = ["pk", "hot", "one", "dups"]


def seg(width):
    return 64 // width


def _sync():
    import torch
    torch.cuda.synchronize()


def _i64(n, off):
    import torch
    return arena_column(None, n, off, dtype=torch.int64)


def make_keys(orc, width, kind, n, nbits, shift):
    """n tuples, payload = row index.
    pk:   a permutation of 1..n (at 10 bits about 4 tuples a digit and tile:
          8-byte tuples never fill a segment, everything travels in the carry
          and is written by the final flush);
    hot:  90 % of the tuples in digit 0;
    one:  every tuple in the last digit (4096 of one digit a tile, every other
          digit empty);
    dups: keys drawn from 1..39."""
    orc.seed(977 + n)
    t = orc.create_relation_pk(n)
    rng = np.random.default_rng(n * 31 + nbits)
    # distinct-ish high parts that keep an 8-byte tuple's key inside int32
    high = (t["key"].astype(np.int64) & 0x3FFFF) << (nbits + shift)
    if kind == "hot":
        hot = rng.random(n) < 0.9
        t["key"][hot] = 1 + high[hot]
    elif kind == "one":
        t["key"] = 1 + (((1 << nbits) - 1) << shift) + high
    elif kind == "dups":
        t["key"] = rng.integers(1, 40, n)
    else:
        assert kind == "pk"
    t["payload"] = np.arange(n)
    return t


def digits_of(t, nbits, shift):
    mask = (((1 << nbits) - 1) << shift) & 0xFFFFFFFF
    return ((t["key"].astype(np.int64) - 1) & mask) >> shift


def content_index(cnt, off):
    """Positions of every partition's tuples in the output, partition by
    partition."""
    cnt, off = np.asarray(cnt, np.int64), np.asarray(off, np.int64)
    packed = np.cumsum(cnt) - cnt
    return np.repeat(off - packed, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)


def run_partition(lib, t, d_in, nbits, shift, padded, cap, want, in_out=(0, 0), io=(1, 3)):
    """One smj_dev_partition into fresh arenas; asserts the record first.
    Returns (tuples of the output view, counts, offsets, arenas)."""
    fan = 1 << nbits
    obuf, d_out = arena(lib, cap, in_out[1])
    hbuf, hist = _i64(fan, io[0])
    fbuf, offs = _i64(fan, io[1])
    lib.dev_partition(d_in, d_out, nbits, shift, padded, hist, offs)
    ran = lib.last_scatter()
    assert ran == want, f"launched {sorted(ran)}, the case is about {sorted(want)}"
    _sync()
    return (lib.to_host(d_out), hist.cpu().numpy(), offs.cpu().numpy(),
            ((obuf, d_out, "out"), (hbuf, hist, "hist"), (fbuf, offs, "off")))


def check_against(got, cnt, off, expect, width, padded, what):
    eout, ecnt, eoff = expect
    assert np.array_equal(cnt, ecnt), f"{what}: counts"
    assert np.array_equal(off, eoff), f"{what}: offsets"
    if padded:
        assert np.all((off * width) % 64 == 0), f"{what}: padded offsets"
    idx = content_index(ecnt, eoff)
    bad = np.flatnonzero(got[idx] != eout[idx])
    if len(bad):
        p = int(np.searchsorted(np.cumsum(ecnt), bad[0], side="right"))
        raise AssertionError(f"{what}: partition {p} differs at output slot {int(idx[bad[0]])}: "
                             f"{got[idx[bad[0]]]} for {eout[idx[bad[0]]]} "
                             f"({len(bad)} of {len(idx)} tuples)")


def both_ways(lib, orc, t, nbits, shift, padded, what, forced_want, plain_want):
    """The case under the switch and without it: the records, and the same
    bytes as the oracle's."""
    n = len(t)
    expect = orc.partition(t, nbits, shift, padded=bool(padded))
    cap = len(expect[0])
    d_in = lib.to_device(t)
    outs = []
    for on, want in ((True, forced_want), (False, plain_want)):
        lib.force_ballot_ranks(on)
        try:
            got, cnt, off, arenas = run_partition(lib, t, d_in, nbits, shift, padded, cap, want)
        finally:
            lib.force_ballot_ranks(False)
        w = f"{what} switch={'on' if on else 'off'}"
        check_against(got, cnt, off, expect, lib.width, padded, w)
        for b, v, name in arenas:
            check_guards(b, v, f"{w}: {name}")
        outs.append(got[content_index(cnt, off)])
    assert np.array_equal(outs[0], outs[1]), f"{what}: ballot and atomic ranks differ"
    assert len(outs[0]) == n


# ---------------------------------------------------------------------------
# ballot ranks with write combining, small sizes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,shift", SWC_DIGITS)
@pytest.mark.parametrize("keys", KEYS)
def test_ballot_wc_small(libs, oracles, width, keys, nbits, shift):
    orc, lib = oracles[width], libs[width]
    sizes = sorted(set(SWC_SIZES + [seg(width) - 1, seg(width)]))
    assert len(sizes) == 10
    for n in sizes:
        t = make_keys(orc, width, keys, n, nbits, shift)
        for padded in (1, 0):       # unpadded: a region's start is not segment aligned
            both_ways(lib, orc, t, nbits, shift, padded,
                      f"{keys} n={n} nbits={nbits} shift={shift} padded={padded}",
                      {"ballot-wc"}, {"atomic"})


def test_key_sets_are_what_they_claim(oracles, width):
    """The properties the cases above rest on (CPU only)."""
    orc = oracles[width]
    n, nbits = 3 * CHUNK + 77, 10
    t = make_keys(orc, width, "pk", n, nbits, 0)
    assert np.array_equal(np.sort(t["key"]), np.arange(1, n + 1))
    # one tile of keys 1..4096: exactly 4 tuples a digit, no full 8-tuple segment
    one_tile = make_keys(orc, width, "pk", TILE, nbits, 0)
    assert np.all(np.bincount(digits_of(one_tile, nbits, 0), minlength=1 << nbits) == 4)
    per_tile = np.bincount(digits_of(t[:TILE], nbits, 0), minlength=1 << nbits)
    assert 3.9 < per_tile.mean() < 4.1 and per_tile.sum() == TILE
    for shift in (0, 3):
        nb = 7 if shift else 10
        d = digits_of(make_keys(orc, width, "hot", n, nb, shift), nb, shift)
        assert 0.88 < np.mean(d == 0) < 0.93
        d = digits_of(make_keys(orc, width, "one", n, nb, shift), nb, shift)
        assert np.all(d == (1 << nb) - 1)
    t = make_keys(orc, width, "dups", n, nbits, 0)
    assert t["key"].min() >= 1 and t["key"].max() <= 39
    big = make_keys(orc, width, "one", 2048 * 2048 + 2049, 12, 0)
    assert big["key"].min() > 0                                # no wrap in 32-bit keys
    assert np.array_equal(big["payload"], np.arange(len(big)))


# ---------------------------------------------------------------------------
# placement under the switch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [4, 10])
def test_ballot_wc_placements(libs, oracles, width, nbits):
    orc, lib = oracles[width], libs[width]
    for n in (TILE + 1, CHUNK + 1):
        t = make_keys(orc, width, "pk", n, nbits, 0)
        for padded in (0, 1):
            expect = orc.partition(t, nbits, 0, padded=bool(padded))
            for oin, oout in ((1, 0), (0, 1), (1, 1), (3, 3)):
                what = f"n={n} nbits={nbits} padded={padded} in+{oin} out+{oout}"
                ibuf, d_in = arena(lib, n, oin, fill=t)
                lib.force_ballot_ranks(True)
                try:
                    got, cnt, off, arenas = run_partition(
                        lib, t, d_in, nbits, 0, padded, len(expect[0]), {"ballot-wc"},
                        in_out=(oin, oout))
                finally:
                    lib.force_ballot_ranks(False)
                check_against(got, cnt, off, expect, width, padded, what)
                assert np.array_equal(lib.to_host(d_in), t), f"{what}: input changed"
                for b, v, name in arenas + ((ibuf, d_in, "in"),):
                    check_guards(b, v, f"{what}: {name}")


# ---------------------------------------------------------------------------
# steady state: every workgroup runs four scatter tiles
# ---------------------------------------------------------------------------
def test_ballot_wc_steady_state(libs, width):
    """n = 2048 * 8192 + 8192 + 1: the smallest size at which a workgroup gets
    a second histogram tile (2048 workgroups of 16384 tuples: four scatter
    tiles each; the last runs 4096 + 4096 + 1).  Against numpy: a stable
    argsort of the digits and the prefix sums of the counts."""
    import torch
    lib = libs[width]
    n, nbits = 2048 * CHUNK + CHUNK + 1, 10
    assert n == 16_785_409
    d_in = lib.empty(n)
    lib.dev_gen_pk(d_in, 0, n, 4242)
    d_in[:, 0] = torch.arange(n, device="cuda", dtype=d_in.dtype)   # payload = row index
    _sync()
    t = lib.to_host(d_in)
    assert np.array_equal(t["payload"], np.arange(n))
    d = digits_of(t, nbits, 0).astype(np.uint16)
    ecnt = np.bincount(d, minlength=1 << nbits).astype(np.int64)
    assert ecnt.sum() == n and ecnt.min() > 0
    eoff = np.cumsum(ecnt) - ecnt
    expect = t[np.argsort(d, kind="stable")]
    hist = torch.full((1 << nbits,), -1, dtype=torch.int64, device="cuda")
    offs = torch.full((1 << nbits,), -1, dtype=torch.int64, device="cuda")
    d_out = lib.empty(n)
    d_out.fill_(0x5A5A5A5A)
    lib.force_ballot_ranks(True)
    try:
        lib.dev_partition(d_in, d_out, nbits, 0, 0, hist, offs)
        assert lib.last_scatter() == {"ballot-wc"}
        _sync()
    finally:
        lib.force_ballot_ranks(False)
    assert np.array_equal(hist.cpu().numpy(), ecnt)
    assert np.array_equal(offs.cpu().numpy(), eoff)
    got = lib.to_host(d_out)
    bad = np.flatnonzero(got != expect)
    assert len(bad) == 0, f"{len(bad)} slots differ, the first at {int(bad[0])}"
    assert np.array_equal(lib.to_host(d_in), t), "input changed"


# ---------------------------------------------------------------------------
# no digit bits: the one route to k_scatter_swc that production takes at small n
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [0, 1])
def test_no_digit_bits(libs, oracles, width, padded):
    orc, lib = oracles[width], libs[width]
    n = CHUNK + 1
    t = make_keys(orc, width, "pk", n, 0, 0)
    expect = orc.partition(t, 0, 0, padded=bool(padded))
    assert expect[1].tolist() == [n] and expect[2].tolist() == [0]
    assert np.array_equal(expect[0][:n], t)
    got, cnt, off, arenas = run_partition(lib, t, lib.to_device(t), 0, 0, padded,
                                          len(expect[0]), {"ballot-wc"})
    check_against(got, cnt, off, expect, width, padded, f"dbits=0 padded={padded}")
    assert np.array_equal(got[:n], t)
    for b, v, name in arenas:
        check_guards(b, v, name)


# ---------------------------------------------------------------------------
# ballot ranks on 256 x 8 tiles (11 and 12 digit bits), without the switch
# ---------------------------------------------------------------------------
T256 = 2048
# 2048 * 2048 + 2049: two 2048-tuple tiles a workgroup
SIZES_256 = [T256 - 1, T256, T256 + 1, 3 * T256 + 77, 2048 * T256 + T256 + 1]


@pytest.mark.parametrize("keys", ["pk", "hot", "one"])
@pytest.mark.parametrize("nbits", [11, 12])
def test_ballot_256x8(libs, oracles, width, nbits, keys):
    orc, lib = oracles[width], libs[width]
    for n in SIZES_256:
        t = make_keys(orc, width, keys, n, nbits, 0)
        d_in = lib.to_device(t)
        for padded in ((1, 0) if n < 10_000 else (1,)):
            what = f"{keys} n={n} nbits={nbits} padded={padded}"
            expect = orc.partition(t, nbits, 0, padded=bool(padded))
            got, cnt, off, arenas = run_partition(lib, t, d_in, nbits, 0, padded,
                                                  len(expect[0]), {"ballot-256x8"})
            check_against(got, cnt, off, expect, width, padded, what)
            for b, v, name in arenas:
                check_guards(b, v, f"{what}: {name}")
    # the switch changes nothing here: these digits never take the atomic ranks
    lib.force_ballot_ranks(True)
    try:
        run_partition(lib, t, d_in, nbits, 0, 1, len(expect[0]), {"ballot-256x8"})
    finally:
        lib.force_ballot_ranks(False)


# ---------------------------------------------------------------------------
# two stable passes (digits wider than 12 bits): 6 + 7 and 7 + 8 bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [CHUNK + 1, 100_003])
@pytest.mark.parametrize("nbits", [13, 15])
def test_two_passes(libs, oracles, width, nbits, n):
    orc, lib = oracles[width], libs[width]
    t = make_keys(orc, width, "pk", n, nbits, 0)
    for padded in (1, 0):
        both_ways(lib, orc, t, nbits, 0, padded, f"n={n} nbits={nbits} padded={padded}",
                  {"two-pass", "ballot-wc"}, {"two-pass", "atomic"})


def test_record_of_nothing(libs, width):
    """A partition of no tuples launches no scatter, and the record says so."""
    import torch
    lib = libs[width]
    hist = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    offs = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    one = lib.empty(1)
    one.fill_(7)
    out = lib.empty(64)
    lib.dev_partition(one, out, 4, 0, 0, hist, offs)   # a record to erase
    assert lib.last_scatter() == {"atomic"}
    _, none = arena(lib, 0, 0)
    lib.dev_partition(none, out, 4, 0, 0, hist, offs)
    assert lib.last_scatter() == set()
    _sync()
    assert hist.cpu().tolist() == [0] * 16 and offs.cpu().tolist() == [0] * 16
