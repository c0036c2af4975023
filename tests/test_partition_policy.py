"""CPU tests of the stable partition's choice of scatter kernel
(csrc/partition_policy.hpp).

stable_partition_narrow and partition_hist_scatter (partition.hip) ask the
header which of four kernels a stable pass launches; SwaGeom, SwcGeom and
scatter_lds take their LDS sizes from it.  Here the header is built alone with
g++ (tests/partition_host) and compared with a restatement, array by array, of
the LDS layouts the kernels' comments give, at both tuple widths; the choice
is checked at the 2^32 boundary of the atomic ranks, under the self-check's
answer and the test switch, and over every digit width for the kernel that no
input selects.
"""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "partition_host", "policy_host.cpp")
ATOMIC, BALLOT_WC, BALLOT_512X16, BALLOT_256X8 = range(4)     # Scatter
LIMIT = 160 * 1024
WIDTHS = (8, 16)
# sizes around every threshold of the choice, and far past it
SIZES = [0, 1, 4096, 1 << 20, (1 << 31) - 1, 1 << 31, (1 << 32) - (64 << 10) - 1,
         (1 << 32) - (64 << 10), (1 << 32) - 129, (1 << 32) - 128, (1 << 32) - 1, 1 << 32,
         (1 << 32) + 1, 1 << 40, (1 << 64) - (64 << 10) - 1]


@pytest.fixture(scope="session")
def policy(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("partition_host") / "libpartition_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           SRC, "-o", out])
    lib = C.CDLL(out)
    u32, u64 = C.c_uint32, C.c_uint64
    lib.pp_stable_scatter_choice.argtypes = [u64, u32, u32, C.c_int, C.c_int]
    lib.pp_ballot_scatter_choice.argtypes = [u32, u32]
    for name in ("pp_swa_lds_bytes", "pp_swc_lds_bytes", "pp_scatter_lds_bytes"):
        getattr(lib, name).argtypes = [u32, u32, u32, u32]
        getattr(lib, name).restype = u64
    lib.pp_swc_max_segs.argtypes = [u32, u32, u32, u32]
    lib.pp_swc_max_segs.restype = u32
    lib.pp_swp_items.argtypes = [u32]
    lib.pp_swp_items.restype = u32
    lib.pp_lds_limit.restype = u64
    lib.pp_scatter_bit.argtypes = [C.c_int]
    lib.pp_scatter_bit.restype = u32
    lib.pp_two_pass_bit.restype = u32
    return lib


def up16(x):
    return (x + 15) // 16 * 16


# ---------------------------------------------------------------------------
# the layout comments of partition.hip, restated piece by piece
# ---------------------------------------------------------------------------
def swc_max_segs(threads, items, tb, nbins):
    """Segments a tile of k_scatter_swc can emit: its tuples and every digit's
    carry (SEG - 1 tuples) in whole segments, a partial first and last one a
    digit."""
    seg = 64 // tb
    return (threads * items + nbins * (seg - 1)) // seg + 2 * nbins


def swc_lds(threads, items, tb, nbins):
    """stage | carry | run | tstart, kc, segpre, emit | wcnt | segown | scratch"""
    seg, waves = 64 // tb, threads // 64
    stage = threads * items * tb
    carry = nbins * (seg - 1) * tb
    run = nbins * 8
    four_u32 = 4 * nbins * 4
    wcnt = waves * nbins * 2
    segown = up16(swc_max_segs(threads, items, tb, nbins) * 2)
    return stage + carry + run + four_u32 + wcnt + segown + 64


def swa_lds(threads, items, tb, nbins):
    """stage | carry [B][CW] | counters u32 [W][B / 2] | info u32x4 [B] |
    segown u16 [TILE / SEG + 2 B] | scratch"""
    seg, waves = 64 // tb, threads // 64
    stage = threads * items * tb
    carry = nbins * (seg - 1) * tb
    counters = waves * (nbins // 2) * 4
    info = nbins * 16
    segown = up16((threads * items // seg + 2 * nbins) * 2)
    return stage + carry + counters + info + segown + 128


def scatter_lds(threads, items, tb, nbins):
    """stage | run u64 | tstart u32 | wcnt u16 [WAVES][nbins] | scratch"""
    return threads * items * tb + nbins * 8 + nbins * 4 + (threads // 64) * nbins * 2 + 64


def test_sizes_match_layout_comments(policy):
    for tb, dbits in itertools.product(WIDTHS, range(13)):
        nbins = 1 << dbits
        where = (tb, dbits)
        assert policy.pp_swc_max_segs(512, 8, tb, nbins) == swc_max_segs(512, 8, tb, nbins), where
        assert policy.pp_swc_lds_bytes(512, 8, tb, nbins) == swc_lds(512, 8, tb, nbins), where
        items = policy.pp_swp_items(tb)
        assert items * tb == 128                       # 64 KiB of tuples a tile
        if 1 <= dbits <= 10:                           # two digits share a counter word
            assert policy.pp_swa_lds_bytes(512, items, tb, nbins) == \
                swa_lds(512, items, tb, nbins), where
        for threads, it in ((512, 16), (256, 8)):
            assert policy.pp_scatter_lds_bytes(threads, it, tb, nbins) == \
                scatter_lds(threads, it, tb, nbins), where
    assert policy.pp_lds_limit() == LIMIT


def test_swc_sizes_at_the_limit(policy):
    """SwcGeom<512, 8>: 1024 bins of 16-byte tuples are 448 bytes below the
    160 KiB a workgroup may ask for; 2048 bins are over it at either width."""
    assert policy.pp_swc_lds_bytes(512, 8, 16, 1024) == 163_392 == LIMIT - 448
    assert policy.pp_swc_lds_bytes(512, 8, 8, 1024) == 138_048
    assert policy.pp_swc_lds_bytes(512, 8, 16, 2048) == 259_136 > LIMIT
    assert policy.pp_swc_lds_bytes(512, 8, 8, 2048) == 242_240 > LIMIT
    # segment numbers and stage offsets travel in 16-bit halves of one scan word
    for tb in WIDTHS:
        assert policy.pp_swc_max_segs(512, 8, tb, 2048) < 1 << 16
    # what each launched kernel asks for fits
    for tb in WIDTHS:
        assert policy.pp_swa_lds_bytes(512, policy.pp_swp_items(tb), tb, 1024) <= LIMIT
        for dbits in (11, 12):
            assert policy.pp_scatter_lds_bytes(256, 8, tb, 1 << dbits) <= LIMIT


def test_atomic_ranks_end_before_2_32(policy):
    """k_scatter_swp keeps positions in 32 bits: for every digit width it
    takes, the last size is 2^32 - (64 << dbits) - 1."""
    for tb, dbits in itertools.product(WIDTHS, range(1, 11)):
        last = (1 << 32) - (64 << dbits) - 1
        assert policy.pp_stable_scatter_choice(last, dbits, tb, 1, 0) == ATOMIC, (tb, dbits)
        assert policy.pp_stable_scatter_choice(last + 1, dbits, tb, 1, 0) == BALLOT_WC, (tb, dbits)


def expected_choice(n, dbits, ok, forced):
    if 1 <= dbits <= 10 and n + (64 << dbits) < 1 << 32 and ok and not forced:
        return ATOMIC
    return BALLOT_WC if dbits <= 10 else BALLOT_256X8


def test_selection(policy):
    n_cases = 0
    for tb, dbits, n, ok, forced in itertools.product(WIDTHS, range(13), SIZES, (0, 1), (0, 1)):
        got = policy.pp_stable_scatter_choice(n, dbits, tb, ok, forced)
        assert got == expected_choice(n, dbits, ok, forced), (tb, dbits, n, ok, forced)
        n_cases += 1
    assert n_cases == 2 * 13 * len(SIZES) * 4
    for tb, dbits in itertools.product(WIDTHS, range(13)):
        # a failed self-check and the switch: write combining up to 10 bits
        want = BALLOT_WC if dbits <= 10 else BALLOT_256X8
        assert policy.pp_stable_scatter_choice(100_003, dbits, tb, 0, 0) == want
        assert policy.pp_stable_scatter_choice(100_003, dbits, tb, 1, 1) == want
        assert policy.pp_stable_scatter_choice(100_003, dbits, tb, 0, 1) == want
        assert policy.pp_ballot_scatter_choice(dbits, tb) == want
    for tb in WIDTHS:
        assert policy.pp_stable_scatter_choice(8193, 0, tb, 1, 0) == BALLOT_WC
        for dbits in (11, 12):
            assert policy.pp_stable_scatter_choice(65536, dbits, tb, 1, 0) == BALLOT_256X8


def test_ballot_512x16_is_unreachable(policy):
    """No input with 0..12 digit bits selects k_scatter<512, 16>: the write-
    combining kernel fits wherever the 512 x 16 tiles would be taken.  A change
    of geometry that tips 16-byte tuples at 1024 bins over the limit would
    select that kernel, which no GPU test runs; this test fails first."""
    seen = set()
    for tb, dbits, n, ok, forced in itertools.product(WIDTHS, range(13), SIZES, (0, 1), (0, 1)):
        seen.add(policy.pp_stable_scatter_choice(n, dbits, tb, ok, forced))
    for tb, dbits in itertools.product(WIDTHS, range(13)):
        seen.add(policy.pp_ballot_scatter_choice(dbits, tb))
    assert seen == {ATOMIC, BALLOT_WC, BALLOT_256X8}
    # why: up to 10 bits the write-combining kernel always fits
    for tb, dbits in itertools.product(WIDTHS, range(11)):
        assert policy.pp_swc_lds_bytes(512, 8, tb, 1 << dbits) <= LIMIT


def test_record_bits_match_header_and_binding(policy):
    """SMJ_SCATTER_* of smj.h, the enum's bits and the binding's names."""
    import smj
    text = open(os.path.join(ROOT, "include", "smj.h")).read()
    defs = {m.group(1): int(m.group(2))
            for m in re.finditer(r"#define SMJ_SCATTER_(\w+)\s+(\d+)u", text)}
    assert defs == {"ATOMIC": 1, "BALLOT_WC": 2, "BALLOT_512X16": 4, "BALLOT_256X8": 8,
                    "TWO_PASS": 16}
    bits = [policy.pp_scatter_bit(s) for s in range(4)] + [policy.pp_two_pass_bit()]
    assert bits == [1, 2, 4, 8, 16]
    assert smj.SCATTERS == ("atomic", "ballot-wc", "ballot-512x16", "ballot-256x8", "two-pass")


def test_library_calls_the_header():
    """partition.hip decides with the header's functions and keeps no second
    copy of the conditions."""
    text = open(os.path.join(PKG, "csrc", "partition.hip")).read()
    assert '#include "partition_policy.hpp"' in text
    assert len(re.findall(r"\bstable_scatter_choice\(", text)) == 2   # assumed ok, then asked
    assert len(re.findall(r"\bballot_scatter_choice\(", text)) == 1
    assert "lds_bytes(1u << dbits) <= 160 * 1024" not in text
    for fn in ("swa_lds_bytes", "swc_lds_bytes", "scatter_lds_bytes", "swc_max_segs"):
        assert re.search(r"\b%s\(" % fn, text), fn
