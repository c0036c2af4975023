"""The device API where the buffers lie, whether they alias and which stream
they are ordered on.

Every other GPU test hands the library fresh allocations (aligned to 256
bytes or more) on the default stream.  Here every buffer is a view into an
arena of sentinels (tests/placement.py) at a tuple offset of 0, 1 or 3: for
8-byte tuples the odd offsets are addresses 8 mod 16, the side of the
library's alignment tests (k_keyrange, the pair stores of the stable
partition, k_hist_v against k_hist_p, the vector form of k_scatter_res) that
aligned buffers never take, and for every kernel without such a test the
proof that it needs none.  smj.h promises no more than the tuple's own
alignment.  Sorts also run in place (out == in: every retry of device_bucket
reads the input again), and a last section runs the entries on a side stream
behind a delayed producer: a launch or copy on any other stream reads stale
zeros.

Expected values are the matrix's (test_gpu_layout_matrix.expected), the
oracle's, and the numpy constructions of test_gpu_join_index and band_ref;
every comparison is bit-exact.
"""
import ctypes

import numpy as np
import pytest

import test_gpu_layout_matrix as M
from band_ref import numpy_band
from placement import GUARD, SENTINEL, arena, arena_column, check_guards
from test_gpu_band_join import check_columns, unchanged
from test_gpu_join_index import check_pairs, numpy_pairs, numpy_semi_mask
from test_gpu_parity import rand_tuples

pytestmark = pytest.mark.gpu

OFFSETS = (0, 1, 3)


def _sync():
    import torch
    torch.cuda.synchronize()


def _int64():
    import torch
    return torch.int64


def _i64(n, off, fill=None):
    """An int64 column (histograms, counts, words) at an element offset."""
    return arena_column(None, n, off, fill=fill, dtype=_int64())


def test_odd_views_are_misaligned(libs, width):
    """What the module rests on: the offsets give the addresses the issue
    names (8-byte tuples: 0, 8 and 24 mod 64; 16-byte: 0, 16 and 48)."""
    lib = libs[width]
    for off in OFFSETS:
        buf, view = arena(lib, 5, off)
        assert buf.data_ptr() % 256 == 0
        assert view.data_ptr() % 64 == (off * width) % 64
        assert view.data_ptr() % 16 == (8 if width == 8 and off % 2 else 0)
        ebuf, empty = arena(lib, 0, off)   # no tuples, and still a place
        assert empty.shape[0] == 0
        assert empty.data_ptr() - ebuf.data_ptr() == view.data_ptr() - buf.data_ptr()


# ---------------------------------------------------------------------------
# sort and join through device_bucket: the matrix under placements
# ---------------------------------------------------------------------------
JOIN_PLACEMENTS = [(1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 1), (3, 1, 1, 3)]
BIG_FIT = 8 * 49152    # 393 216: eight times every layout's scatter tile


def big_fit(row):
    """The row's layout at 393 216 x 393 216 dense tuples, where every sampled
    layout completes (all shards level, module docstring of the matrix): the
    scatters of the narrow layouts themselves read the odd input.  D1 = 8,
    D2 = 0, s1 = 11."""
    flags, pay, hinted, e8, e16 = M.A_ROWS[row]
    c = M.Case(f"P-{row}-big_fit", "join", BIG_FIT, BIG_FIT, 8, flags,
               (1, BIG_FIT) if hinted else None, M.dense_keys, pay, {8: e8, 16: e16},
               why="no such layout for 8-byte tuples")
    c.key_span = {8: (1, BIG_FIT), 16: (1, BIG_FIT)}
    return c


@pytest.mark.parametrize("placement", JOIN_PLACEMENTS, ids=lambda p: "".join(map(str, p)))
@pytest.mark.parametrize("row", list(M.A_ROWS))
def test_join_placements(libs, oracles, width, row, placement):
    """Every forced layout at fit, tile, d2_2 and the 393 216-tuple shape,
    with (R_in, S_in, R_out, S_out) at the given tuple offsets.  The layout a
    call ends in is the table's: a placement does not change it."""
    cases = M.group_a(row, ["fit", "tile", "d2_2"]) + [big_fit(row)]
    M.run_cases(libs, oracles, width, cases, placement)


def keyrange_case(name, nR, nS, fanout):
    """An unhinted join at flags 0: device_bucket takes the exact key range
    first (k_keyrange), here 1..nR, and plans from it as from a hint.  Row
    ids fit the 32-bit words of that plan (tile: s1 = 10, d2_2: s1 = 12), and
    with the narrower range (the hinted shapes plan from max(nR, nS)) the
    partitions are half the table's.  They stay inside their shards, but for
    d2_2 in 8-byte tuples: S's 70 001 words fill five scatter tiles of 16384,
    on shards 0 to 4 alone, a region overflows, and the call goes on to the
    sampled tuples, whose six tiles of 12288 fit.  The test runs the case
    with aligned buffers too: the layout is the same."""
    e8 = "tuples" if name == "d2_2" else "p32"
    c = M.Case(f"P-keyrange-{name}", "join", nR, nS, fanout, 0, None, M.dense_keys, "rowid",
               {8: e8, 16: "p32"})
    c.key_span = {8: (1, nR), 16: (1, nR)}
    return c


@pytest.mark.parametrize("shape", ["tile", "d2_2"])
def test_keyrange_scalar_and_vector_branch(libs, oracles, width, shape):
    """k_keyrange with R at offset 1 (8-byte tuples: its scalar branch) and S
    at offset 0 (the vector branch) in one launch."""
    name, nR, nS, fan = next(s for s in M.A_SHAPES if s[0] == shape)
    case = keyrange_case(name, nR, nS, fan)
    M.run_cases(libs, oracles, width, [case])   # aligned: the same layout
    M.run_cases(libs, oracles, width, [case], (1, 0, 0, 1))


SORT_PLACEMENTS = {"in_odd": (1, 0), "out_odd": (0, 1), "inplace0": ("inplace", 0),
                   "inplace1": ("inplace", 1)}


@pytest.mark.parametrize("placement", list(SORT_PLACEMENTS))
@pytest.mark.parametrize("row", list(M.C_ROWS))
def test_sort_placements(libs, oracles, width, row, placement):
    """Group C under an odd input, an odd output and in place (out is in) at
    offsets 0 and 1."""
    M.run_cases(libs, oracles, width, M.group_c(row), SORT_PLACEMENTS[placement])


def retry_chain_cases():
    """In-place sorts whose call discards attempts before it finishes; every
    attempt reads `in` again, so none may have written `out`."""
    out = []
    # full-width payloads at flags 0: the 32-bit words fail on them, then the
    # 48-bit planes; 16-byte tuples go on to the 12-byte elements (C's p96
    # row), 8-byte tuples stay: 48 - s1 = 37 bits hold any 32-bit payload
    c = M.Case("P-full-49229", "sort", 49229, 49229, 0, 0, None, M.dense_keys, "full",
               {8: "p48", 16: "p96"})
    out.append(c)
    # a shard region overflows in every sampled attempt: "tuples!"
    out += [c for row in ("p32", "p96", "tuples") for c in M.group_c(row) if c.nR == 4096]
    # keys that break the size guess 1..n: the sort re-plans from the exact range
    names = {"B-s1_1-600000-sort", "B-s1_31_fit-1100-sort", "B-s1_32_fit-1100-sort",
             "B-full8-600000-sort", "B-l64_fit-1100-sort"}
    out += [c for c in M.group_b() if c.name in names]
    return out


_RETRY = retry_chain_cases()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("case", _RETRY, ids=lambda c: c.name)
def test_inplace_sort_through_retries(libs, oracles, width, case, off):
    assert case.kind == "sort"
    if case.name.startswith("B-"):
        assert case.keys_break_guess
    M.run_cases(libs, oracles, width, [case], ("inplace", off))


# ---------------------------------------------------------------------------
# smj_dev_partition
# ---------------------------------------------------------------------------
def scatter_tile(width):
    """The scatter tile of stable_partition_swp."""
    return 8192 if width == 8 else 4096


_PART = {}


def partition_expected(orc, width, n, nbits, shift, padded):
    key = (width, n, nbits, shift, padded)
    if key not in _PART:
        orc.seed(12345 + n)
        t = orc.create_relation_pk(n)
        t["payload"] = np.arange(n) + 5
        _PART[key] = (t,) + orc.partition(t, nbits, shift, padded=bool(padded))
    return _PART[key]


@pytest.mark.parametrize("nbits,shift", [(4, 0), (10, 0), (7, 3)])
@pytest.mark.parametrize("which", ["one", "tile-1", "2tiles+77", "100003"])
def test_partition_placements(libs, oracles, width, which, nbits, shift):
    import torch
    orc, lib = oracles[width], libs[width]
    T = scatter_tile(width)
    n = {"one": 1, "tile-1": T - 1, "2tiles+77": 2 * T + 77, "100003": 100_003}[which]
    fan = 1 << nbits
    for padded in (0, 1):
        t, eout, ecnt, eoff = partition_expected(orc, width, n, nbits, shift, padded)
        for oin, oout in ((1, 0), (0, 1), (1, 1), (3, 3)):
            what = f"partition n={n} nbits={nbits} shift={shift} padded={padded} in+{oin} out+{oout}"
            ibuf, d_in = arena(lib, n, oin, fill=t)
            obuf, d_out = arena(lib, len(eout), oout)
            hbuf, hist = _i64(fan, 1)
            fbuf, offs = _i64(fan, 3)
            lib.dev_partition(d_in, d_out, nbits, shift, padded, hist, offs)
            _sync()
            cnt, off = hist.cpu().numpy(), offs.cpu().numpy()
            assert np.array_equal(cnt, ecnt), what
            assert np.array_equal(off, eoff), what
            got = lib.to_host(d_out)
            for i in range(fan):
                assert np.array_equal(got[off[i]:off[i] + cnt[i]],
                                      eout[eoff[i]:eoff[i] + ecnt[i]]), f"{what}: partition {i}"
            assert np.array_equal(lib.to_host(d_in), t), f"{what}: input changed"
            for b, v, name in ((ibuf, d_in, "in"), (obuf, d_out, "out"), (hbuf, hist, "hist"),
                               (fbuf, offs, "off")):
                check_guards(b, v, f"{what}: {name}")


# ---------------------------------------------------------------------------
# the range partitions and the segmented joins of the multi-GPU exchange
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["tuples", "words"])
@pytest.mark.parametrize("nbits", [3, 10])
@pytest.mark.parametrize("n", [4097, 65536 + 511])
@pytest.mark.parametrize("form", ["sampled", "shards"])
def test_partition_range_placements(libs, oracles, width, form, n, nbits, packed):
    """smj_dev_partition_range_sampled and _shards (the latter against
    _packed's words) with the input and the tuple or word output at offset 1:
    the checks of test_partition_range_sampled_small_bits and
    test_partition_range_shards."""
    from test_gpu_parity import partition_range_sampled_case, partition_range_shards_case
    if packed and width != 16:
        pytest.skip("packed words are the 16-byte layout")
    case = partition_range_sampled_case if form == "sampled" else partition_range_shards_case
    case(libs[width], oracles[width], nbits, n, packed, in_off=1, out_off=1)


@pytest.mark.parametrize("nbits", [3, 10])
@pytest.mark.parametrize("n", [4097, 65536 + 511])
def test_partition_range_exact_placements(libs, oracles, width, n, nbits):
    """smj_dev_partition_range and _packed with the input, the output and the
    histogram at offset 1, against the plain definition: partition p holds
    exactly the tuples with keys in [1 + p * 2^s1, 1 + (p + 1) * 2^s1), in
    any order (plan_partition: every bucket is sorted afterwards); a packed
    word is (key offset in the partition) << (64 - s1) | payload (smj.h)."""
    import torch
    from smj.dist import plan_shift
    orc, lib = oracles[width], libs[width]
    orc.seed(7 + n + nbits)
    t = orc.create_relation_fk(n, 5 * n)
    t["payload"] = np.arange(n)
    kmax, F = 5 * n, 1 << nbits
    s1 = plan_shift(1, kmax, nbits)
    rel = t["key"].astype(np.int64) - 1
    digit = np.minimum(rel >> s1, F - 1)
    order = np.argsort(digit, kind="stable")
    want_hist = np.bincount(digit, minlength=F)
    ibuf, d_in = arena(lib, n, 1, fill=t)
    obuf, out = arena(lib, n, 1)
    hbuf, hist = _i64(F, 1)
    lib.dev_partition_range(d_in, out, nbits, 1, kmax, hist)
    _sync()
    assert np.array_equal(hist.cpu().numpy(), want_hist)
    ends = np.cumsum(want_hist)
    got = lib.to_host(out)
    for p in range(F):   # the payloads are the row ids: each partition in their order
        part = got[ends[p] - want_hist[p]:ends[p]]
        assert np.array_equal(part[np.argsort(part["payload"])],
                              t[order][ends[p] - want_hist[p]:ends[p]]), f"partition {p}"
    guards = [(ibuf, d_in, "in"), (obuf, out, "out"), (hbuf, hist, "hist")]
    if width == 16:
        wbuf, words = _i64(n, 1)
        h2buf, hist2 = _i64(F, 3)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert 1 <= s1 <= 32
        assert lib.dev_partition_range_packed(d_in, words, nbits, 1, kmax, hist2, bad)
        _sync()
        assert int(bad.item()) == 0
        assert np.array_equal(hist2.cpu().numpy(), want_hist)
        want = ((rel & ((1 << s1) - 1)).astype(np.uint64) << np.uint64(64 - s1)) | \
            t["payload"].astype(np.uint64)
        gotw = words.cpu().numpy().view(np.uint64)
        for p in range(F):
            a, b = ends[p] - want_hist[p], ends[p]
            assert np.array_equal(np.sort(gotw[a:b]), np.sort(want[order][a:b])), f"words {p}"
        guards += [(wbuf, words, "words"), (h2buf, hist2, "hist of the words")]
    assert np.array_equal(lib.to_host(d_in), t)
    for buf, view, name in guards:
        check_guards(buf, view, f"partition_range n={n} nbits={nbits}: {name}")


@pytest.mark.parametrize("nbits", [3, 10])
@pytest.mark.parametrize("n", [4097, 65536 + 511])
def test_partition_range_planes_placements(libs, oracles, width, n, nbits):
    """smj_dev_partition_range_planes with its input at offset 1 (the planes
    keep their documented alignment): it applies, flags nothing it should not,
    keeps every region inside smj_sampled_capacity(), and the words decoded
    from the regions (test_gpu_dist.planes_tuples) are the input, each key in
    its partition.  4097 tuples are one scatter tile and an odd tail; at 2^3
    partitions the per-region slack is tightest."""
    import torch
    from smj.dist import Planes, plan_shift
    from test_gpu_dist import planes_tuples
    orc, lib = oracles[width], libs[width]
    orc.seed(99 + n)
    t = orc.create_relation_pk(n)
    t["payload"] = np.arange(n)[::-1]
    F, K = 1 << nbits, lib.sampled_shards()
    s1 = plan_shift(1, n, nbits)
    assert 1 <= s1 <= 32 and n < 1 << (48 - s1)
    cap = lib.sampled_capacity(n, nbits)
    ibuf, d_in = arena(lib, n, 1, fill=t)
    out = Planes(-(-cap // 32) * 32 + 32, device="cuda")   # 32 spare elements a plane
    for plane in out.planes:
        plane.fill_(-7)
    ss = torch.empty(F * K, dtype=torch.int64, device="cuda")
    sc = torch.empty(F * K, dtype=torch.int64, device="cuda")
    fl = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    assert lib.dev_partition_range_planes(d_in, out.buf, out.stride, nbits, 1, n, ss, sc, fl)
    _sync()
    assert np.array_equal(lib.to_host(d_in), t), "input changed"
    check_guards(ibuf, d_in, f"partition_range_planes n={n} nbits={nbits}: in")
    for plane in out.planes:
        assert bool((plane[cap:] == -7).all()), "wrote past the capacity"
    flags = fl.tolist()
    assert flags[1] == 0, "a clean input was flagged not packable"
    if flags[0]:
        # a region overflowed, as in test_partition_range_sampled_small_bits
        # (few workgroups fill few of a partition's shards): the caller
        # repeats with exact regions; nothing passed the buffer
        return
    ssh, sch = ss.cpu().numpy(), sc.cpu().numpy()
    assert int(sch.sum()) == n
    assert int((ssh + sch).max()) <= cap and int(ssh.min()) >= 0
    assert np.all((ssh + sch)[:-1] <= ssh[1:]), "regions overlap"
    got = planes_tuples(out, ss, sc, K, s1)
    part = np.repeat(np.arange(F * K) // K, sch)
    assert np.array_equal(np.minimum((got[:, 0] - 1) >> s1, F - 1), part)
    want = np.stack([t["key"].astype(np.int64), t["payload"].astype(np.int64)], 1)
    assert np.array_equal(got[np.argsort(got[:, 0])], want[np.argsort(want[:, 0])])


@pytest.mark.parametrize("packed", [False, True], ids=["tuples", "words"])
def test_segmented_join_placements(libs, oracles, width, packed):
    """smj_dev_partition_range / _packed into odd outputs and
    smj_dev_join_segmented on receive buffers at offset 1 (its scratch, used
    in place): world = 3 of test_segmented_join_simulated_exchange."""
    from test_gpu_dist import segmented_exchange_case
    if packed and width != 16:
        pytest.skip("packed words are the 16-byte layout")
    segmented_exchange_case(libs[width], oracles[width], 3, "pk_fk", packed, off=1)


@pytest.mark.parametrize("layout", ["tuples", "words", "planes"])
def test_segmented_tables_placements(libs, oracles, width, layout):
    """smj_dev_partition_range_sampled / _planes from an odd input and
    smj_dev_join_segmented_tables on odd receive buffers: world = 3 of
    test_sampled_exchange_simulated (the planes stay aligned)."""
    from test_gpu_dist import sampled_exchange_case
    if layout == "words" and width != 16:
        pytest.skip("packed words are the 16-byte layout")
    sampled_exchange_case(libs[width], oracles[width], 3, "pk_fk", layout, False, off=1)


# ---------------------------------------------------------------------------
# merges
# ---------------------------------------------------------------------------
_MERGE2 = {}


@pytest.mark.parametrize("offs", [(1, 1, 1), (1, 0, 0), (0, 1, 1), (0, 0, 1)],
                         ids=lambda o: "".join(map(str, o)))
@pytest.mark.parametrize("la,lb", [(1, 1), (2047, 2050), (70_000, 33_333)])
def test_merge2_placements(libs, oracles, width, la, lb, offs):
    orc, lib = oracles[width], libs[width]
    if (width, la, lb) not in _MERGE2:
        a = orc.sort(rand_tuples(width, la, la, 0, 5000))
        b = orc.sort(rand_tuples(width, lb, lb + 1, 0, 5000))
        _MERGE2[width, la, lb] = (a, b, orc.merge(a, b))
    a, b, exp = _MERGE2[width, la, lb]
    abuf, da = arena(lib, la, offs[0], fill=a)
    bbuf, db = arena(lib, lb, offs[1], fill=b)
    obuf, out = arena(lib, la + lb, offs[2])
    lib.dev_merge2(da, db, out)
    _sync()
    assert np.array_equal(lib.to_host(out), exp)
    assert np.array_equal(lib.to_host(da), a) and np.array_equal(lib.to_host(db), b)
    for buf, v, name in ((abuf, da, "a"), (bbuf, db, "b"), (obuf, out, "out")):
        check_guards(buf, v, f"merge2 {la}+{lb} at {offs}: {name}")


_RUNS = {}


def ragged_runs(orc, width, k):
    """k sorted runs of 0..maxlen tuples, every fifth one empty, and what
    their merge is."""
    if (width, k) not in _RUNS:
        rng = np.random.default_rng(k)
        maxlen = 3000 if k <= 64 else 300
        lens = [0 if i % 5 == 2 else int(rng.integers(1, maxlen)) for i in range(k)]
        runs = [orc.sort(rand_tuples(width, n, 100 * k + i, 0, 10000)) for i, n in enumerate(lens)]
        _RUNS[width, k] = (runs, orc.multiway_merge(runs))
    return _RUNS[width, k]


def run_table_in_arena(lib, view, lens):
    """Library.run_table for consecutive pieces of one device view (empty
    pieces keep their place's pointer)."""
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    k = len(lens)
    ptrs = (ctypes.c_void_p * k)(*[view.data_ptr() + int(s) * lib.width for s in starts])
    clen = (ctypes.c_uint64 * k)(*[int(n) for n in lens])
    table = (ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(clen, ctypes.c_void_p), k,
             (ptrs, clen))
    return table, [view.data_ptr() + int(s) * lib.width for s in starts]


@pytest.mark.parametrize("k", [3, 64, 257])
def test_multiway_merge_placements(libs, oracles, width, k):
    """The runs are consecutive ragged pieces of one arena, so their starts
    fall on every parity; the output is odd."""
    orc, lib = oracles[width], libs[width]
    runs, exp = ragged_runs(orc, width, k)
    lens = [len(r) for r in runs]
    data = np.concatenate(runs)
    rbuf, rview = arena(lib, len(data), 1, fill=data)
    table, ptrs = run_table_in_arena(lib, rview, lens)
    if width == 8:
        assert {p % 16 for p in ptrs} == {0, 8}
    obuf, out = arena(lib, len(exp), 1)
    lib.dev_multiway_merge(table, out)
    _sync()
    assert np.array_equal(lib.to_host(out), exp)
    assert np.array_equal(lib.to_host(rview), data), "runs changed"
    check_guards(rbuf, rview, f"multiway merge k={k}: runs")
    check_guards(obuf, out, f"multiway merge k={k}: out")


# ---------------------------------------------------------------------------
# merge-join count, materialize, pairs, semi / anti, band
# ---------------------------------------------------------------------------
BANDS = [(0, 0), (-3, 5)]
_SORTED = {}


def sorted_pair(orc, width, nR, nS):
    """Sorted R and S with duplicates (keys uniform in 1..n/4) and what every
    entry point has to give for them."""
    key = (width, nR, nS)
    if key not in _SORTED:
        R = orc.sort(rand_tuples(width, nR, nR, 1, max(nR // 4, 1) + 1))
        S = orc.sort(rand_tuples(width, nS, nS + 1, 1, max(nS // 4, 1) + 1))
        for a in (R, S):
            a.setflags(write=False)
        r_idx, s_idx = numpy_pairs(R, S)
        assert len(r_idx) == orc.merge_join(R, S)
        mat = S[s_idx]
        if len(mat) < 1 << 20:
            assert np.array_equal(mat, orc.merge_join_materialize(R, S))
        band = {b: numpy_band(R["key"], S["key"], *b) for b in BANDS}
        _SORTED[key] = dict(R=R, S=S, r_idx=r_idx, s_idx=s_idx, mask=numpy_semi_mask(R, S),
                            band=band)
    return _SORTED[key]


def family(f):
    """R and S at odd offsets, over the sizes that cross MT_TILE = 512,
    MT_RWIN = 1024 and kMatPiece = 8192.  At most 137 S tiles: the scan's
    blocks of 1024 tiles are test_gpu_join_blocks.py's."""
    f = pytest.mark.parametrize("offR,offS", [(1, 0), (0, 1), (1, 1)])(f)
    return pytest.mark.parametrize("nR,nS", [(1, 1), (1025, 2049), (40_001, 70_001)])(f)


class SortedOnDevice:
    """The sorted pair of a case on the device at its offsets, the outputs a
    test asks for (each in an arena of its own), and at the end the checks
    that hold for every entry point: inputs unchanged, every guard intact."""

    def __init__(self, lib, orc, nR, nS, offR, offS):
        self.lib = lib
        self.e = sorted_pair(orc, lib.width, nR, nS)
        self.R, self.S = self.e["R"], self.e["S"]
        self.what = f"nR={nR} nS={nS} R+{offR} S+{offS}"
        rbuf, self.dR = arena(lib, nR, offR, fill=self.R)
        sbuf, self.dS = arena(lib, nS, offS, fill=self.S)
        self.guards = [(rbuf, self.dR, "R"), (sbuf, self.dS, "S")]

    def out(self, total, short, off, tuples=False):
        """(view of `total` places at offset `off`, what the call gets, its
        capacity): all of them, or with `short` the first total - 1 (None: the
        capacity is 0 and the call only counts)."""
        buf, view = (arena if tuples else arena_column)(self.lib, total, off)
        cap = total - 1 if short else total
        self.guards.append((buf, view, f"output of {total} at +{off}, short={short}"))
        return view, (view[:cap] if cap > 0 else None), cap

    def last_untouched(self, view, short):
        if short and view.shape[0]:
            assert bool((view[-1:] == SENTINEL).all()), f"{self.what}: wrote past out_cap"

    def finish(self):
        _sync()
        unchanged(self.lib, self.dR, self.dS, self.R, self.S)
        for buf, view, name in self.guards:
            check_guards(buf, view, f"{self.what}: {name}")


@family
def test_merge_join_count_placements(libs, oracles, width, nR, nS, offR, offS):
    d = SortedOnDevice(libs[width], oracles[width], nR, nS, offR, offS)
    cbuf, count = arena_column(None, 1, 1, dtype=_int64())
    d.guards.append((cbuf, count, "count"))
    count.fill_(1000)
    d.lib.dev_merge_join_count(d.dR, d.dS, count)
    _sync()
    assert int(count.item()) == 1000 + len(d.e["r_idx"]), d.what   # added, not written
    d.finish()


@family
def test_materialize_placements(libs, oracles, width, nR, nS, offR, offS):
    """Tuple output at offset 1; then out_cap = total - 1."""
    d = SortedOnDevice(libs[width], oracles[width], nR, nS, offR, offS)
    want = d.S[d.e["s_idx"]]
    for short in (False, True):
        view, out, cap = d.out(len(want), short, 1, tuples=True)
        assert d.lib.dev_materialize(d.dR, d.dS, out) == len(want), d.what
        _sync()
        assert np.array_equal(d.lib.to_host(view)[:cap], want[:cap]), f"{d.what} short={short}"
        d.last_untouched(view, short)
    d.finish()


@family
def test_join_pairs_placements(libs, oracles, width, nR, nS, offR, offS):
    """Payload and key columns at element offsets 1, 3 and 1; then out_cap =
    total - 1."""
    d = SortedOnDevice(libs[width], oracles[width], nR, nS, offR, offS)
    r_idx, s_idx = d.e["r_idx"], d.e["s_idx"]
    for short in (False, True):
        cols = [d.out(len(r_idx), short, o) for o in (1, 3, 1)]
        cap = cols[0][2]
        args = [c[1] for c in cols] if cap > 0 else []
        assert d.lib.dev_join_pairs(d.dR, d.dS, *args) == len(r_idx), d.what
        _sync()
        check_pairs([c[0].cpu().numpy()[:cap] for c in cols], d.R, d.S, r_idx, s_idx)
        for view, _, _ in cols:
            d.last_untouched(view, short)
    d.finish()


@pytest.mark.parametrize("anti", [False, True], ids=["semi", "anti"])
@family
def test_semi_join_placements(libs, oracles, width, nR, nS, offR, offS, anti):
    d = SortedOnDevice(libs[width], oracles[width], nR, nS, offR, offS)
    m = ~d.e["mask"] if anti else d.e["mask"]
    n = int(m.sum())
    for short in (False, True):
        view, out, cap = d.out(n, short and n > 0, 1, tuples=True)
        assert d.lib.dev_semi_join(d.dR, d.dS, out, anti=anti) == n, d.what
        _sync()
        assert np.array_equal(d.lib.to_host(view)[:cap], d.S[m][:cap]), f"{d.what} short={short}"
        d.last_untouched(view, short)
    d.finish()


@pytest.mark.parametrize("band", BANDS, ids=lambda b: f"{b[0]}..{b[1]}")
@family
def test_band_join_placements(libs, oracles, width, nR, nS, offR, offS, band):
    """smj_dev_band_join into four columns at element offsets 1, 3, 3 and 1
    (then with out_cap = total - 1) and smj_dev_band_join_count."""
    d = SortedOnDevice(libs[width], oracles[width], nR, nS, offR, offS)
    r_idx, s_idx = d.e["band"][band]
    total = len(r_idx)
    for short in (False, True):
        cols = [d.out(total, short and total > 0, o) for o in (1, 3, 3, 1)]
        cap = cols[0][2]
        args = [c[1] for c in cols] if cap > 0 else []
        assert d.lib.dev_band_join(d.dR, d.dS, band[0], band[1], *args) == total, d.what
        _sync()
        check_columns([c[0].cpu().numpy()[:cap] for c in cols], d.R, d.S, r_idx, s_idx)
        for view, _, _ in cols:
            d.last_untouched(view, short)
    cbuf, count = arena_column(None, 1, 3, dtype=_int64())
    d.guards.append((cbuf, count, "count"))
    count.fill_(7)
    d.lib.dev_band_join_count(d.dR, d.dS, band[0], band[1], count)
    _sync()
    assert int(count.item()) == 7 + total, d.what
    d.finish()


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
GEN_TOTAL, GEN_FIRST, GEN_N = 65_537, 12_345, 20_001


def _generate(lib, kind, out, first, total):
    if kind == "pk":
        lib.dev_gen_pk(out, first, total, 12345)
    elif kind == "fk":
        lib.dev_gen_fk(out, first, total, 33_333, 54321)
    elif kind == "zipf":
        lib.dev_gen_zipf(out, first, 100_000, 0.75, 54321)
    elif kind == "nonunique":
        lib.dev_gen_nonunique(out, first, total, 33_333, 4242, 3)
    else:
        lib.dev_gen_zipf_ref(out, first, 100_000, 0.75, 4242, 3)


@pytest.mark.parametrize("kind", ["pk", "fk", "zipf", "nonunique", "zipf_ref"])
def test_generator_shard_placements(libs, width, kind):
    """A shard with an odd first index, an odd length and an odd output offset
    equals [first, first + n) of the relation generated once into an aligned
    buffer."""
    lib = libs[width]
    whole = lib.empty(GEN_TOTAL)
    _generate(lib, kind, whole, 0, GEN_TOTAL)
    _sync()
    want = lib.to_host(whole)[GEN_FIRST:GEN_FIRST + GEN_N]
    assert len(np.unique(want["key"])) > 100
    for off in (1, 3):
        buf, out = arena(lib, GEN_N, off)
        _generate(lib, kind, out, GEN_FIRST, GEN_TOTAL)
        _sync()
        assert np.array_equal(lib.to_host(out), want), f"{kind} shard at +{off}"
        check_guards(buf, out, f"{kind} shard at +{off}")


# ---------------------------------------------------------------------------
# the reference's flow on device memory
# ---------------------------------------------------------------------------
def _partition_relation_device(lib, d_in, d_out, n, nbits):
    """partition_relation (unpadded) through the ctypes handle on device
    pointers: (counts, start offsets in tuples)."""
    import smj
    fan = 1 << nbits
    rin, rout = smj.Relation(d_in.data_ptr(), n), smj.Relation(d_out.data_ptr(), n)
    rels, ptrs = lib._parts(fan)
    lib.lib.partition_relation(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.byref(rin),
                               ctypes.byref(rout), nbits, 0)
    cnt = [int(rels[i].num_tuples) for i in range(fan)]
    off = [(int(rels[i].tuples or d_out.data_ptr()) - d_out.data_ptr()) // lib.width
           for i in range(fan)]
    return cnt, off


def _sorted_by_reference_flow(lib, orc, t, seed_off):
    """partition_relation, avxsort_tuples of every partition where it lies
    (one of them scalarsort_tuples in place), avx_multiway_merge of the runs:
    all on device pointers.  Returns the merged device relation's arena."""
    import smj
    n, nbits = len(t), 4
    fan = 1 << nbits
    ibuf, d_in = arena(lib, n, seed_off, fill=t)
    pbuf, d_part = arena(lib, n, 1)
    sbuf, d_sort = arena(lib, n, 1)
    _sync()   # the reference-named entries run on the library's own stream
    cnt, off = _partition_relation_device(lib, d_in, d_part, n, nbits)
    _sync()
    _, ecnt, eoff = orc.partition(t, nbits, 0, padded=False)
    assert cnt == ecnt.tolist() and off == eoff.tolist()
    if lib.width == 8:
        assert {(d_part.data_ptr() + o * 8) % 16 for o in off} == {0, 8}, "runs of every parity"
    inplace = max(range(fan), key=lambda i: cnt[i])
    for i in range(fan):
        src = d_part.data_ptr() + off[i] * lib.width
        dst = d_sort.data_ptr() + off[i] * lib.width
        if i == inplace:
            # scalarsort_tuples sorts in place (scalarsort.c:41-50): copy the
            # partition to its place in the second buffer and sort it there
            d_sort[off[i]:off[i] + cnt[i]].copy_(d_part[off[i]:off[i] + cnt[i]])
            _sync()
            pa, pb = ctypes.c_void_p(dst), ctypes.c_void_p(src)
            lib.lib.scalarsort_tuples(ctypes.byref(pa), ctypes.byref(pb), cnt[i])
            where = pb.value   # the pointers are swapped: *outputptr is the sorted input
        else:
            pa, pb = ctypes.c_void_p(src), ctypes.c_void_p(dst)
            lib.lib.avxsort_tuples(ctypes.byref(pa), ctypes.byref(pb), cnt[i])
            where = pb.value
        assert where == dst or cnt[i] == 0, f"partition {i}: the sorted run is not in the output"
    _sync()
    part_h = lib.to_host(d_part)
    got = lib.to_host(d_sort)
    for i in range(fan):
        assert np.array_equal(got[off[i]:off[i] + cnt[i]],
                              orc.sort(part_h[off[i]:off[i] + cnt[i]])), f"partition {i}"
    check_guards(sbuf, d_sort, "sorted partitions")
    check_guards(pbuf, d_part, "partitions")
    # avx_multiway_merge over the device runs
    mbuf, d_out = arena(lib, n, 1)
    rels = (smj.Relation * fan)(*[smj.Relation(d_sort.data_ptr() + off[i] * lib.width, cnt[i])
                                  for i in range(fan)])
    ptrs = (ctypes.POINTER(smj.Relation) * fan)(*[ctypes.pointer(rels[i]) for i in range(fan)])
    fifo = np.zeros(1 << 16, lib.dtype)
    got_n = lib.lib.avx_multiway_merge(d_out.data_ptr(), ctypes.cast(ptrs, ctypes.c_void_p), fan,
                                       fifo.ctypes.data, len(fifo))
    _sync()
    assert got_n == n
    for i in range(fan):  # parts[i] consumed as documented (avx_multiwaymerge.c:268-272)
        assert rels[i].num_tuples == 0
        assert rels[i].tuples == d_sort.data_ptr() + (off[i] + cnt[i]) * lib.width
    assert np.array_equal(lib.to_host(d_out), orc.sort(t))
    check_guards(mbuf, d_out, "merged relation")
    check_guards(ibuf, d_in, "input")
    assert np.array_equal(lib.to_host(d_in), t)
    return d_out, mbuf


def test_reference_flow_on_device_memory(libs, oracles, width):
    """The reference's join thread on device pointers: partition, sort every
    partition where it lies, merge the runs, merge-join two such relations."""
    orc, lib = oracles[width], libs[width]
    n = 100_003
    rels = []
    for seed, off in ((12345, 1), (54321, 0)):
        orc.seed(seed)
        t = orc.create_relation_nonunique(n, n // 3)
        rels.append((t,) + _sorted_by_reference_flow(lib, orc, t, off))
    (tR, dR, _), (tS, dS, _) = rels
    got = int(lib.lib.merge_join(dR.data_ptr(), dS.data_ptr(), n, n, None))
    assert got == orc.merge_join(orc.sort(tR), orc.sort(tS))


# ---------------------------------------------------------------------------
# a side stream behind a delayed producer
# ---------------------------------------------------------------------------
_SLEEP = {}


def _sleep_cycles(ms):
    """torch.cuda._sleep cycles of about `ms` milliseconds, measured once."""
    import torch
    if "per_ms" not in _SLEEP:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)   # the first call sets the kernel up
        probe = 20_000_000
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        _SLEEP["per_ms"] = probe / max(a.elapsed_time(b), 1e-3)
    return int(_SLEEP["per_ms"] * ms)


def side_stream(lib, inputs, call, warm=None):
    """Runs call(views) on a side stream whose inputs arrive late.

    inputs: [(structured array or int64 array, offset)]; every view is
    pre-filled with zeros (stale but valid tuples).  On the stream: an
    optional warm(views) on the stale data (a first call that may grow the
    workspace), a delay of about 50 ms, the real data copied into the views,
    call(views) -> tensors to clone (all on the stream), and only then a
    synchronisation.  Returns (host copies of the clones, whether the stream
    was still busy when call returned, the views' arenas).  A kernel or copy
    issued on any other stream runs before the data arrives and reads zeros.
    The default stream stays idle throughout."""
    import torch
    cycles = _sleep_cycles(50)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        placed, staged = [], []
        for data, off in inputs:
            if data.dtype.names:
                buf, view = arena(lib, len(data), off)
                src = lib.to_device(data)
            else:
                buf, view = _i64(len(data), off)
                src = torch.from_numpy(np.array(data)).cuda()
            view.zero_()
            placed.append((buf, view))
            staged.append(src)
        views = [v for _, v in placed]
        if warm is not None:
            warm(views)
        s.synchronize()   # everything above is setup; nothing below waits
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(s)
        torch.cuda._sleep(cycles)
        t1.record(s)
        for view, src in zip(views, staged):
            if view.shape[0]:
                view.copy_(src, non_blocking=True)
        outs = call(views)
        busy = not s.query()
        clones = [o.clone() for o in outs]
        s.synchronize()
    delay = t0.elapsed_time(t1)
    assert delay >= 5.0, f"the producer's delay was only {delay:.2f} ms"
    for buf, view in placed:
        check_guards(buf, view, "side stream input")
    return [c.cpu().numpy() for c in clones], busy, placed


def _tuples(lib, a):
    return a.reshape(-1).view(lib.dtype)


def _mid_case(row="p32"):
    return next(c for c in M.group_a(row, ["d2_2"]))


def test_stream_dev_sort(libs, oracles, width):
    lib = libs[width]
    case = next(c for c in M.group_c("p32") if c.nR == 49229)
    rels, srt, _ = M.expected(case, width, oracles[width])
    lib.reset_workspace()

    def call(v):
        buf, out = arena(lib, case.nR, 1)
        lib.dev_sort(v[0], out)
        return [out, buf]
    (got, buf), _, _ = side_stream(lib, [(rels[0], 1)], call)
    assert np.array_equal(_tuples(lib, got), srt[0])
    assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all()


@pytest.mark.parametrize("hinted", [True, False], ids=["hinted", "unhinted"])
def test_stream_dev_join(libs, oracles, width, hinted):
    import torch
    lib = libs[width]
    case = _mid_case() if hinted else keyrange_case("d2_2", 40_000, 70_001, 4)
    rels, srt, cnt = M.expected(case, width, oracles[width])
    lib.reset_workspace()

    def call(v):
        outs = [arena(lib, len(t), 1)[1] for t in rels]
        count = torch.full((1,), 0x7EADBEEF, dtype=torch.int64, device="cuda")
        lo, hi = case.hint if hinted else (1, 0)
        lib.dev_join(v[0], v[1], outs[0], outs[1], count, case.fanout, lo, hi)
        return outs + [count]
    (gR, gS, gc), _, _ = side_stream(lib, [(rels[0], 1), (rels[1], 0)], call)
    assert int(gc[0]) == cnt
    assert np.array_equal(_tuples(lib, gR), srt[0]) and np.array_equal(_tuples(lib, gS), srt[1])


def test_stream_dev_partition(libs, oracles, width):
    orc, lib = oracles[width], libs[width]
    n, nbits, shift = 100_003, 7, 3
    t, eout, ecnt, eoff = partition_expected(orc, width, n, nbits, shift, 0)

    def call(v):
        out = arena(lib, n, 1)[1]
        hist, offs = _i64(1 << nbits, 1)[1], _i64(1 << nbits, 3)[1]
        lib.dev_partition(v[0], out, nbits, shift, 0, hist, offs)
        return [out, hist, offs]
    (got, cnt, off), _, _ = side_stream(lib, [(t, 1)], call)
    assert np.array_equal(cnt, ecnt) and np.array_equal(off, eoff)
    assert np.array_equal(_tuples(lib, got), eout[:n])


def test_stream_dev_merge2(libs, oracles, width):
    orc, lib = oracles[width], libs[width]
    la, lb = 70_000, 33_333
    a = orc.sort(rand_tuples(width, la, la, 0, 5000))
    b = orc.sort(rand_tuples(width, lb, lb + 1, 0, 5000))

    def call(v):
        out = arena(lib, la + lb, 1)[1]
        lib.dev_merge2(v[0], v[1], out)
        return [out]
    (got,), _, _ = side_stream(lib, [(a, 1), (b, 1)], call)
    assert np.array_equal(_tuples(lib, got), orc.merge(a, b))


def test_stream_dev_multiway_merge_does_not_wait(libs, oracles, width):
    """k = 64: stream-ordered and, as smj.h promises, without a host
    synchronisation: the stream is still busy with the producer's delay when
    the call returns."""
    orc, lib = oracles[width], libs[width]
    runs, exp = ragged_runs(orc, width, 64)
    lens = [len(r) for r in runs]
    data = np.concatenate(runs)
    scratch = {}

    def merge(v):
        table, _ = run_table_in_arena(lib, v[0], lens)
        out = arena(lib, len(exp), 1)[1]
        lib.dev_multiway_merge(table, out)
        scratch["keep"] = table
        return [out]
    (got,), busy, _ = side_stream(lib, [(data, 1)], merge, warm=merge)
    assert np.array_equal(_tuples(lib, got), exp)
    assert busy, "smj_dev_multiway_merge_host waited for the stream"


def test_stream_counts_do_not_wait(libs, oracles, width):
    """smj_dev_merge_join_count and the second smj_dev_band_join_count on a
    workspace: right results behind the delay, and the stream is still busy
    when each returns."""
    import torch
    orc, lib = oracles[width], libs[width]
    e = sorted_pair(orc, width, 1025, 2049)
    lo, hi = BANDS[1]
    state = {}

    def warm(v):
        c = torch.zeros(1, dtype=torch.int64, device="cuda")
        lib.dev_band_join_count(v[0], v[1], lo, hi, c)   # the first call on the workspace

    def call(v):
        c1 = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        c2 = torch.full((1,), 9, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream()
        lib.dev_merge_join_count(v[0], v[1], c1)
        state["busy_mj"] = not s.query()
        lib.dev_band_join_count(v[0], v[1], lo, hi, c2)
        state["busy_band"] = not s.query()
        return [c1, c2]
    lib.reset_workspace()
    (c1, c2), _, _ = side_stream(lib, [(e["R"], 1), (e["S"], 1)], call, warm=warm)
    assert int(c1[0]) == 5 + len(e["r_idx"])
    assert int(c2[0]) == 9 + len(e["band"][lo, hi][0])
    assert state["busy_mj"], "smj_dev_merge_join_count waited for the stream"
    assert state["busy_band"], "smj_dev_band_join_count waited for the stream"


def test_stream_dev_join_pairs(libs, oracles, width):
    orc, lib = oracles[width], libs[width]
    e = sorted_pair(orc, width, 1025, 2049)
    R, S, r_idx, s_idx = e["R"], e["S"], e["r_idx"], e["s_idx"]
    total = len(r_idx)
    state = {}

    def call(v):
        cols = [arena_column(lib, total, o)[1] for o in (1, 3, 1)]
        state["total"] = lib.dev_join_pairs(v[0], v[1], *cols)
        return cols
    (r, s, k), _, _ = side_stream(lib, [(R, 1), (S, 1)], call)
    assert state["total"] == total
    assert np.array_equal(r, R["payload"][r_idx]) and np.array_equal(s, S["payload"][s_idx])
    assert np.array_equal(k, S["key"][s_idx])


def test_stream_generator(libs, width):
    """The output is zeroed on the stream behind the delay and generated
    after that: a generator launched on another stream is overwritten."""
    lib = libs[width]
    whole = lib.empty(GEN_TOTAL)
    _generate(lib, "pk", whole, 0, GEN_TOTAL)
    _sync()
    want = lib.to_host(whole)[GEN_FIRST:GEN_FIRST + GEN_N]
    stale = np.zeros(GEN_N, lib.dtype)

    def call(v):
        _generate(lib, "pk", v[0], GEN_FIRST, GEN_TOTAL)
        return [v[0]]
    (got,), _, _ = side_stream(lib, [(stale, 1)], call)
    assert np.array_equal(_tuples(lib, got), want)
