"""The level-1 sampled scatter (k_scatter_res) in steady state.

The layout matrix stops at 392 K tuples, where every scatter workgroup gets
one tile: the loop that prefetches tile t + 1 under the stores of tile t never
goes round.  The sizes here give every workgroup several tiles:

* 13 000 003 and 13 000 002 tuples a relation: more than 3 x 256 x the largest
  scatter tile (16 384), so each of the (at most 256) workgroups runs several
  tiles, the last workgroup fewer, the last tile is partial, and the even size
  takes the 8-byte build's 16-byte pair loads;
* 256 x tile + 1 for the tile of the layout under test: two tiles a
  workgroup, and a last workgroup whose only tile holds one tuple.

Every intermediate layout the scatter serves is forced with set_layouts and a
payload that fits it, as bench.py's --payload does, through the join and the
one-relation sort.  Inputs come from the device generators (R: a permutation
of the keys 1..n, S: uniform draws from them), so the match count is n.  The
outputs are checked on the device with the order test and the
order-independent checksum of bench.py's output_check, restated here.

One more case makes the sampled regions overflow at the large size, so that
the fallback to the exact partition is taken from a multi-tile scatter."""
import pytest
import torch

NO_P48, NO_PACKED, NO_SAMPLED, SAMPLE_PLAN, NO_P32, NO_P96 = 1, 2, 4, 8, 16, 32
FANOUT = 8  # bench.py's default: 256 level-1 partitions at these sizes

# layout: (flags, payload kind, widths, scatter tile at 256 partitions by width)
LAYOUTS = {
    "p32": (0, "low16", (8, 16), {8: 16 * 1024, 16: 8 * 1024}),
    "p48": (NO_P32, "rowid", (8, 16), {8: 12 * 1024, 16: 8 * 1024}),
    "words": (NO_P32 | NO_P48, "wide48", (16,), {16: 8 * 1024}),
    "p96": (0, "full64", (16,), {16: 6 * 1024}),
    "tuples": (NO_PACKED | NO_P96, "rowid", (8, 16), {8: 12 * 1024, 16: 4 * 1024}),
}
SIZES = ("odd", "even", "tile+1")


def size_of(kind, layout, width):
    if kind == "odd":
        return 13_000_003
    if kind == "even":
        return 13_000_002
    return 256 * LAYOUTS[layout][3][width] + 1


def test_sizes_give_several_tiles():
    """The sizes against the scatter's chunking (scatter_chunk, partition.hip):
    at most 256 workgroups, each a whole number of tiles."""
    for layout, (_, _, widths, tiles) in LAYOUTS.items():
        for w in widths:
            tile = tiles[w]
            for kind in ("odd", "even"):
                n = size_of(kind, layout, w)
                assert n > 3 * 256 * 16384
                ntiles = -(-n // tile)
                per_wg = -(-ntiles // 256)
                assert per_wg >= 4
                assert n % tile != 0                      # the last tile is partial
                assert ntiles % per_wg != 0               # the last workgroup gets fewer
            n = size_of("tile+1", layout, w)
            ntiles = -(-n // tile)
            assert ntiles == 257 and -(-ntiles // 256) == 2 and n - 256 * tile == 1


# ---- bench.py's output_check, restated --------------------------------------
def checksum(t):
    """Order-independent checksum of (n, 2) rows (payload, key): wrapping
    int64 sums of the keys, the payloads and two avalanche hashes of each row."""
    k = t[:, 1].to(torch.int64)
    p = t[:, 0].to(torch.int64)
    z = (k * 0x2545F4914F6CDD1D) ^ (p + 0x632BE59BD9B4E019)
    z = (z ^ (z >> 31)) * 0x1B873593CA5A7E35
    z = (z ^ (z >> 29)) * 0x3C79AC492BA7B653
    z = z ^ (z >> 32)
    return torch.stack([k.sum(), p.sum(), z.sum(), (z * (z | 1)).sum()])


def is_sorted(t, w):
    """(key, payload) ascending; 8-byte tuples compare as the signed 64-bit
    word key << 32 | unsigned payload."""
    if t.shape[0] < 2:
        return True
    k = t[:, 1].to(torch.int64)
    p = t[:, 0].to(torch.int64)
    if w == 8:
        p = p & 0xFFFFFFFF
    ok = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (p[1:] >= p[:-1]))
    return bool(ok.all().item())


def check_output(src, out, w, what):
    assert is_sorted(out, w), f"{what}: not in (key, payload) order"
    assert torch.equal(checksum(src), checksum(out)), f"{what}: not a permutation of its input"


# ---- inputs ------------------------------------------------------------------
def set_payload(t, kind, salt):
    """low16: 16 bits of the row id (what a 32-bit word keeps beside the keys
    of these sizes, s1 <= 16); rowid: as generated; wide48: 2^40 + row id;
    full64: a 64-bit hash of the row id, negative for half the rows."""
    if kind == "rowid":
        return
    i = torch.arange(t.shape[0], dtype=torch.int64, device=t.device)
    if kind == "low16":
        t[:, 0] = (i & 0xFFFF).to(t.dtype)
    elif kind == "wide48":
        t[:, 0] = i + (1 << 40)
    else:
        assert kind == "full64"
        z = (i + salt) * -7046029254386353131
        z = (z ^ (z >> 31)) * 0x1B873593CA5A7E35
        t[:, 0] = z ^ (z >> 29)


def relations(lib, n, pay):
    R, S = lib.empty(n), lib.empty(n)
    lib.dev_gen_pk(R, 0, n, 12345)
    lib.dev_gen_fk(S, 0, n, n, 54321)
    set_payload(R, pay, 0)
    set_payload(S, pay, 1 << 62)
    torch.cuda.synchronize()
    return R, S


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("op", ["join", "sort"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_scatter_steady_state(libs, width, layout, size, op):
    flags, pay, widths, _ = LAYOUTS[layout]
    if width not in widths:
        pytest.skip("no such layout for 8-byte tuples")
    lib = libs[width]
    n = size_of(size, layout, width)
    what = f"{op} {layout} w{width} n={n}"
    R, S = relations(lib, n, pay)
    keep = [R.clone(), S.clone()]
    lib.reset_workspace()
    lib.set_layouts(flags)
    try:
        sR = lib.empty(n)
        if op == "join":
            sS = lib.empty(n)
            count = torch.full((1,), 0x7EADBEEF, dtype=torch.int64, device="cuda")
            lib.dev_join(R, S, sR, sS, count, FANOUT, 1, n)
            torch.cuda.synchronize()
            # S draws its keys from R's, which are the keys 1..n once each
            assert int(count.item()) == n, f"{what}: count {int(count.item())} != {n}"
            check_output(keep[1], sS, width, what + " S")
            assert torch.equal(S, keep[1]), f"{what}: input S changed"
        else:
            lib.dev_sort(R, sR)
            torch.cuda.synchronize()
        check_output(keep[0], sR, width, what + " R")
        assert torch.equal(R, keep[0]), f"{what}: input R changed"
        assert lib.last_layout() == layout, f"{what}: layout {lib.last_layout()}"
    finally:
        lib.set_layouts(0)
        lib.reset_workspace()


def overflow_keys(n, seed_shift):
    """Keys 1..n's range, arranged so that the sampled regions overflow.  The
    region sizes come from a blocked sample (k_sample_hist: 4 tuples at every
    512th position).  All tuples lie in partition 0 of 256 (keys 1..2^16 under
    the plan of the hint 1..n: s1 = 16) except the sampled ones, which are
    spread over the other partitions: the estimate of partition 0 is zero,
    its shard regions hold their slack of 1024 elements, and every workgroup
    overflows them with its first tile."""
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    hot = 1 + (i * 40503 + seed_shift) % 65536
    cold = 65537 + (i // 512 * 4 + i % 4 + seed_shift) % (n - 65536)
    return torch.where(i % 512 < 4, cold, hot)


@gpu
def test_overflow_after_several_tiles(libs, width):
    """The reservation is read on the overflow path too: a 13 000 003-tuple
    join whose sampled attempts (48-bit planes, then tuples) overflow and
    which ends in the exact partition with the right answer."""
    lib = libs[width]
    n = 13_000_003
    dt = torch.int32 if width == 8 else torch.int64
    rels = []
    for shift in (0, 7):
        t = lib.empty(n)
        t[:, 1] = overflow_keys(n, shift).to(dt)
        t[:, 0] = torch.arange(n, dtype=torch.int64, device="cuda").to(dt)
        rels.append(t)
    R, S = rels
    assert int(((R[:, 1].to(torch.int64) - 1) >> 16 == 0).sum().item()) > n - n // 100
    cR = torch.bincount(R[:, 1].to(torch.int64), minlength=n + 1)
    cS = torch.bincount(S[:, 1].to(torch.int64), minlength=n + 1)
    want = int((cR * cS).sum().item())
    keep = [R.clone(), S.clone()]
    lib.reset_workspace()
    lib.set_layouts(NO_P32)
    try:
        sR, sS = lib.empty(n), lib.empty(n)
        count = torch.full((1,), 0x7EADBEEF, dtype=torch.int64, device="cuda")
        lib.trace(True)
        lib.dev_join(R, S, sR, sS, count, FANOUT, 1, n)
        torch.cuda.synchronize()
        trace = lib.trace_read()
        lib.trace(False)
        ran = {k for k, (_, launches) in trace.items() if launches > 0}
        assert int(count.item()) == want, f"count {int(count.item())} != {want}"
        check_output(keep[0], sR, width, "overflow R")
        check_output(keep[1], sS, width, "overflow S")
        assert torch.equal(R, keep[0]) and torch.equal(S, keep[1])
        assert "k_scatter" in ran, sorted(ran)
        # the sampled attempts overflowed: the exact partition's histogram ran
        assert "k_hist" in ran, sorted(ran)
        assert lib.last_layout() == "tuples"
    finally:
        lib.trace(False)
        lib.set_layouts(0)
        lib.reset_workspace()
