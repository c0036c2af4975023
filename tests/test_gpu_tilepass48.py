"""The tile pass of 48-bit words with its two planes staged in turn
(k_tilepass48): two 16384-element tiles share a compute unit,
and the second plane (the uint16 plane of the 8-byte build, the byte plane of
the 16-byte one) leaves LDS as whole dwords except at the two ends of a tile,
where a dword may belong in part to the neighbour tile.

Every join here is checked against the oracle: the count and both sorted
relations, bit for bit.  The 32-bit words are switched off (LAYOUT_NO_P32) so
that the small inputs take the 48-bit planes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 16384
# segment lengths around the thread, dword and tile boundaries
EDGES = [1, 3, 4, 5, 1023, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 7]
# the segmented joins: keys 1..2^21 in 4 exchanged partitions (level-1 buckets)
KEY_LO, KEY_HI, BUCKET_BITS = 1, 1 << 21, 2
S1 = 21 - BUCKET_BITS  # make_plan: the bit length of the key span less D1
N_SEG = 1_100_000      # level-2 digits: ceil_log2(N_SEG / 2048) - 2 = 8 bits
D2 = 8
S2 = S1 - D2


@pytest.fixture
def p48(libs, width):
    import smj
    lib = libs[width]
    lib.set_layouts(smj.LAYOUT_NO_P32)
    try:
        yield lib
    finally:
        lib.set_layouts(0)


def _relation(orc, keys, payload):
    t = np.zeros(len(keys), orc.dtype)
    t["key"] = keys
    t["payload"] = payload
    return t


def _words(rel):
    """LayP48 words of the segmented plan: (key - KEY_LO) mod 2^s1 in the top
    s1 of 48 bits, the payload below."""
    k = rel["key"].astype(np.int64)
    pay = rel["payload"].astype(np.int64).view(np.uint64)
    assert not (pay >> np.uint64(48 - S1)).any()
    r = (k - KEY_LO).astype(np.uint64)
    return ((r & np.uint64((1 << S1) - 1)) << np.uint64(48 - S1)) | pay


def _lay_out(rel, order, seg_lens, base):
    """Planes holding rel[order] (rows grouped by partition) in the segments
    seg_lens[p] (a list per partition, summing to the partition's size), back
    to back from element offset `base`; returns (planes, start, cnt, starts of
    all tiles)."""
    import torch
    from smj.dist import Planes
    nb = 1 << BUCKET_BITS
    nseg = max(len(s) for s in seg_lens)
    start = np.zeros((nb, nseg), np.int64)
    cnt = np.zeros((nb, nseg), np.int64)
    pos, tiles = base, []
    for p in range(nb):
        for j, c in enumerate(seg_lens[p]):
            start[p, j], cnt[p, j] = pos, c
            tiles += list(range(pos, pos + c, TILE))
            pos += c
        start[p, len(seg_lens[p]):] = pos
    n = len(rel)
    assert pos == base + n
    w = _words(rel[order])
    stride = -(-(pos + 5) // 32) * 32
    lo = np.full(stride, -7, np.int32)
    hi = np.full(stride, -7, np.int16)
    lo[base:pos] = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    hi[base:pos] = (w >> np.uint64(32)).astype(np.uint16).view(np.int16)
    pl = Planes(stride, device="cuda")
    pl.lo.copy_(torch.from_numpy(lo))
    pl.hi.copy_(torch.from_numpy(hi))
    return pl, torch.from_numpy(start).cuda(), torch.from_numpy(cnt).cuda(), np.array(tiles)


def _by_partition(rel):
    part = (rel["key"].astype(np.int64) - KEY_LO) >> S1
    order = np.argsort(part, kind="stable")
    return order, np.bincount(part, minlength=1 << BUCKET_BITS)


def _join_planes(lib, orc, R, S, layR, layS):
    import torch
    exp, eR, eS = orc.sortmergejoin(R, S)
    (pR, stR, ctR, _), (pS, stS, ctS, _) = layR, layS
    sR, sS = lib.empty(len(R)), lib.empty(len(S))
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib.dev_join_segmented_planes(pR.buf, pR.stride, len(R), stR, ctR, pS.buf, pS.stride,
                                  len(S), stS, ctS, BUCKET_BITS, KEY_LO, KEY_HI, sR, sS, cnt)
    torch.cuda.synchronize()
    assert int(cnt.item()) == exp, (int(cnt.item()), exp)
    assert np.array_equal(lib.to_host(sR), eR)
    assert np.array_equal(lib.to_host(sS), eS)


def _uniform_inputs(orc, seed):
    rng = np.random.default_rng(seed)
    span = KEY_HI - KEY_LO + 1
    kR = rng.permutation(span)[:N_SEG].astype(np.int64) + KEY_LO
    kS = rng.integers(KEY_LO, KEY_HI + 1, N_SEG)
    R = _relation(orc, kR, np.arange(N_SEG) + 5)
    S = _relation(orc, kS, np.arange(N_SEG)[::-1] + 1)
    return R, S


def test_tile_edges(p48, oracles, width):
    """Segments of 1 .. 2 * 16384 + 7 elements back to back, starting at
    element offsets 0, 1, 2 and 3 mod 4: neighbouring tiles (of neighbouring
    segments, and of R's and S's different bases) share dwords of the second
    plane, and every tile shape from one element to a full tile occurs."""
    orc, lib = oracles[width], p48
    R, S = _uniform_inputs(orc, 2024)
    lays = []
    for rel, base in ((R, 0), (S, 3)):
        order, sizes = _by_partition(rel)
        seg_lens = []
        for p, c in enumerate(sizes):
            lens = EDGES[p:] + EDGES[:p]  # another order in every partition
            assert c > sum(lens)
            seg_lens.append(lens + [int(c) - sum(lens)])
        lay = _lay_out(rel, order, seg_lens, base)
        lays.append(lay)
    tiles = np.concatenate([lays[0][3], lays[1][3]])
    assert set(tiles % 4) == {0, 1, 2, 3}
    _join_planes(lib, orc, R, S, *lays)


def test_degenerate_digits(p48, oracles, width):
    """One full tile of S whose keys all share one level-2 digit (one run, the
    whole tile; its group goes to the skew path), next to tiles in which
    every one of the 2^D2 digits occurs, and the first and the last bucket
    (the digit path that does not assume keys inside the plan) holding the
    first and the last key of the range.  Keys outside a hint cannot reach
    this kernel in a word: the partition flags them and the join runs again
    with the exact range (test_both_planes_carry_payload's third call)."""
    orc, lib = oracles[width], p48
    R, S = _uniform_inputs(orc, 77)
    # both ends of the range: in R exactly once, in S at least once
    S["key"][:2] = (KEY_LO, KEY_HI)
    R = R[(R["key"] != KEY_LO) & (R["key"] != KEY_HI)]
    R = np.concatenate([R, _relation(orc, [KEY_LO, KEY_HI], [3, 4])])
    # the hot tile: TILE tuples of S in digit 5 of partition 1
    k0 = KEY_LO + (1 << S1) + (5 << S2)
    hot = np.random.default_rng(5).integers(k0, k0 + (1 << S2), TILE)
    S = np.concatenate([_relation(orc, hot, np.arange(TILE) + N_SEG + 1), S])
    lays = []
    for rel in (R, S):
        order, sizes = _by_partition(rel)  # stable: the hot tuples lead partition 1
        seg_lens = [[int(c) // 2, int(c) - int(c) // 2] for c in sizes]
        if rel is S:
            seg_lens[1] = [TILE, int(sizes[1]) - TILE]
            first = rel[order][sizes[0]:sizes[0] + TILE]
            digit = ((first["key"].astype(np.int64) - KEY_LO) >> S2) & ((1 << D2) - 1)
            assert (digit == 5).all()
            nxt = rel[order][sizes[0] + TILE:sizes[0] + 2 * TILE]
            digit = ((nxt["key"].astype(np.int64) - KEY_LO) >> S2) & ((1 << D2) - 1)
            assert len(np.unique(digit)) == 1 << D2
        lays.append(_lay_out(rel, order, seg_lens, 0))
    _join_planes(lib, orc, R, S, *lays)


def test_both_planes_carry_payload(p48, oracles, width):
    """dev_join of 500 000 x 500 000 with a key-range hint and payloads that
    reach the word's last payload bit (2^8 partitions of keys 0..n: s1 = 11,
    so 37 payload bits; 8-byte tuples: all 31 bits of a non-negative int32),
    twice on one workspace; then once with a hint the keys leave, which the
    48-bit words cannot hold (the join falls back to the exact range)."""
    import torch
    orc, lib = oracles[width], p48
    n = 500_000
    orc.seed(12345)
    R = orc.create_relation_mway(n, n)
    orc.seed(54321)
    S = orc.create_relation_nonunique(n, n)
    for rel in (R, S):
        row = np.arange(n, dtype=np.int64)
        h = (row * 2654435761 >> 7)
        if width == 16:
            rel["payload"] = row + ((h % 32) << 32)
            assert int(rel["payload"].max()) >> 36 == 1
        else:
            rel["payload"] = (row + ((h % 2048) << 20)).astype(np.int32)
            assert int(rel["payload"].max()) >> 30 == 1
    exp, eR, eS = orc.sortmergejoin(R, S)
    dR, dS = lib.to_device(R), lib.to_device(S)
    sR, sS = lib.empty(n), lib.empty(n)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib.reset_workspace()
    import smj
    lib.set_layouts(smj.LAYOUT_NO_P32)
    for call, key_max in enumerate((n, n, n // 2)):
        sR.zero_()
        sS.zero_()
        lib.dev_join(dR, dS, sR, sS, cnt, 8, 0, key_max)  # S's keys start at 0
        torch.cuda.synchronize()
        assert int(cnt.item()) == exp, call
        assert np.array_equal(lib.to_host(sR), eR), call
        assert np.array_equal(lib.to_host(sS), eS), call
        if call < 2:
            assert lib.last_layout() == "p48", (call, lib.last_layout())


@pytest.mark.parametrize("d2_bits", [0, 8, 10])
def test_two_tiles_share_a_compute_unit(libs, width, d2_bits):
    """The occupancy query of the 48-bit tile-pass kernel at its launch's LDS
    size: losing the second resident workgroup (a VGPR too many, a larger
    stage) would cost the overlap and fail nothing else."""
    assert libs[width].tilepass_occupancy("p48", d2_bits) >= 2
    assert libs[width].tilepass_occupancy("p32", d2_bits) >= 2
    assert libs[width].tilepass_occupancy("tuples", d2_bits) == -1
