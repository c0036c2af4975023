// groupagg.hip -- grouped aggregation of one sorted relation (smj.h
// smj_dev_group_aggregate): one output row per maximal run of equal
// key >> group_shift, with the run's first key, start, length and the sum,
// minimum and maximum of its payloads.  The library's own; the reference has
// joins only.
//
// A run does not respect tile boundaries (a hot key spans thousands of
// tiles), and no workgroup may wait for another, so the passes are the
// project's count -> scan -> write with one more step over the tiles only:
//   k_group_count one workgroup per tile of GA_TILE elements, every wave a
//                 chunk of GA_CHUNK consecutive ones (lane l of round j holds
//                 element 64 j + l of it).  Element i is a head when i == 0 or
//                 its group differs from that of element i - 1 (the first
//                 element of a chunk reads one key in front of it).  Leaves
//                 the tile's number of heads and its open tail: the
//                 aggregate from its last head to its end (of the whole tile
//                 when it has no head) and that head's position, or none;
//   k_mat_scan    materialize.hip's, over the head counts: the heads in front
//                 of every tile, which number its rows, and the total;
//   k_group_carry a segmented scan of the tails over the tiles (three small
//                 kernels over ntiles items, GC_BLOCK tiles a workgroup): for
//                 every tile the aggregate and the start of the part of the
//                 group open at its first element that lies in earlier
//                 tiles.  A tile without a head passes its predecessor's
//                 carry on, combined with its own;
//   k_group_write one workgroup per tile: reads the tile again, forms the
//                 inclusive aggregates of the runs with a segmented scan over
//                 the lanes of each round, carried from round to round in
//                 registers and from wave to wave through LDS, and writes a
//                 row at every element that ends its group (the next element
//                 is a head or lies behind the relation; the last element of
//                 a chunk reads one key behind it).  The row of a group is
//                 the rank of its head, so consecutive ends -- consecutive
//                 lanes -- write consecutive rows of every column.  An end
//                 whose head lies in front of its chunk combines what came in
//                 from the earlier waves and the tile's carry.
// Where a head lies and how many precede a lane come from the rounds' head
// ballots; only sum, minimum and maximum go through the scan.  With a group
// shift the first key of a run is not the key of its end: the end reads it
// from the relation at the run's start (one key per row, not a pass).
// smj_dev_group_count is the count pass over the keys alone and a reduction.
// What window.hip's kernels use as well (the geometry, GAgg and GCarry, the
// lane moves, ga_load, ga_seg_scan, gc_block_scan) lies in ga_common.hpp.
#include "smj_common.hpp"
#include "smj_internal.hpp"
#include "mat_common.hpp"
#include "ga_common.hpp"

namespace smj {

uint32_t group_tile() { return GA_TILE; }

// the output columns (each may be null)
struct GroupCols {
    MatVal* key;
    int64_t* start;
    int64_t* count;
    int64_t* sum;
    MatVal* mn;
    MatVal* mx;
};

struct GWave {  // what a wave leaves for the others of its tile
    GCarry tail;
    uint32_t heads;
};

// AGG 0: the tails' head positions alone (tail may be null: the count form),
// 1: with their sums, 2: with minimum and maximum as well (what nobody asks
// for is not computed: the scans are what the passes spend their time on).
template <int AGG>
__global__ void __launch_bounds__(GA_THREADS)
k_group_count(const Tup* __restrict__ in, uint64_t n, uint32_t gsh, uint64_t* __restrict__ cnt,
              GCarry* __restrict__ tail) {
    __shared__ GWave L[GA_WAVES];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint64_t cb = (uint64_t)blockIdx.x * GA_TILE + (uint64_t)w * GA_CHUNK;
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    uint32_t heads = 0;
    uint64_t lstart = kNoHead;  // the chunk's last head
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        heads += (uint32_t)__popcll(hb[j]);
        if (hb[j]) lstart = cb + 64 * j + top_bit(hb[j]);
    }
    GAgg a = ga_none();
    if (AGG) {
#pragma unroll
        for (int j = 0; j < GA_IPT; j++) {
            const uint64_t gi = cb + 64 * j + lane;
            // behind the last head, or everything (kNoHead is above every gi)
            const bool in_tail = gi < n && (lstart == kNoHead || gi >= lstart);
            if (in_tail) a = ga_comb(a, GAgg{(int64_t)pay[j], pay[j], pay[j]});
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            a = ga_comb(a, GAgg{sh_xor(a.sum, o), sh_xor(a.mn, o), sh_xor(a.mx, o)});
    }
    if (lane == 0) {
        L[w].tail = GCarry{a.sum, AGG == 2 ? (int64_t)a.mn : 0, AGG == 2 ? (int64_t)a.mx : 0,
                           lstart};
        L[w].heads = heads;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        GCarry t = gc_none();
        uint64_t h = 0;
#pragma unroll
        for (int v = 0; v < GA_WAVES; v++) {
            t = gc_comb(t, L[v].tail);
            h += L[v].heads;
        }
        cnt[blockIdx.x] = h;
        if (tail) tail[blockIdx.x] = t;
    }
}

// ---- the carry step: a segmented scan of the tails over the tiles

// per GC_BLOCK tiles: their tails combined
__global__ void __launch_bounds__(GC_BLOCK)
k_group_carry_part(const GCarry* __restrict__ tail, uint64_t ntiles, GCarry* __restrict__ part) {
    __shared__ GCarry wl[GC_BLOCK / 64];
    const uint64_t t = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    GCarry all;
    gc_block_scan(t < ntiles ? tail[t] : gc_none(), wl, &all);
    if (threadIdx.x == 0) part[blockIdx.x] = all;
}

// pexcl[b] = the parts in front of workgroup b combined (one workgroup)
__global__ void __launch_bounds__(GC_BLOCK)
k_group_carry_pscan(const GCarry* __restrict__ part, uint32_t nb, GCarry* __restrict__ pexcl) {
    __shared__ GCarry wl[GC_BLOCK / 64];
    GCarry run = gc_none();
    if (threadIdx.x == 0) pexcl[0] = run;
    for (uint32_t r0 = 0; r0 < nb; r0 += GC_BLOCK) {
        const uint32_t b = r0 + threadIdx.x;
        GCarry all;
        const GCarry inc = gc_block_scan(b < nb ? part[b] : gc_none(), wl, &all);
        if (b + 1 < nb) pexcl[b + 1] = gc_comb(run, inc);
        run = gc_comb(run, all);
    }
}

// carry[t] = the tails of all tiles in front of tile t combined
__global__ void __launch_bounds__(GC_BLOCK)
k_group_carry_down(const GCarry* __restrict__ tail, uint64_t ntiles,
                   const GCarry* __restrict__ pexcl, GCarry* __restrict__ carry) {
    __shared__ GCarry wl[GC_BLOCK / 64];
    const uint64_t t = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    GCarry all;
    const GCarry inc = gc_block_scan(t < ntiles ? tail[t] : gc_none(), wl, &all);
    const GCarry front = pexcl[blockIdx.x];
    if (t == 0) carry[0] = front;
    if (t + 1 < ntiles) carry[t + 1] = gc_comb(front, inc);
}

// AGG 0: key, start and count alone, 1: the sum too, 2: minimum and maximum too
template <int AGG>
__global__ void __launch_bounds__(GA_THREADS)
k_group_write(const Tup* __restrict__ in, uint64_t n, uint32_t gsh,
              const uint64_t* __restrict__ base, const GCarry* __restrict__ carry,
              GroupCols cols, uint64_t out_cap) {
    __shared__ GWave L[GA_WAVES];
    const uint64_t row0 = base[blockIdx.x];  // the heads in front of the tile
    // the tile's first row is row0 - 1 (a group open at its first element)
    // or row0: nothing below out_cap (uniform over the workgroup)
    if (row0 > out_cap) return;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint64_t cb = (uint64_t)blockIdx.x * GA_TILE + (uint64_t)w * GA_CHUNK;
    const uint64_t le = lanemask_le();
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    // is the element behind the chunk a head (the relation's end counts)
    const uint64_t ce = cb + GA_CHUNK;
    bool next_head = ce == n;
    if (ce < n) next_head = (ga_key(in + ce) >> gsh) != (ga_key(in + ce - 1) >> gsh);

    GAgg x[GA_IPT];        // aggregate from the element's head, or the chunk's start, to it
    uint64_t st[GA_IPT];   // that head's position; kNoHead: in front of the chunk
    uint32_t hrank[GA_IPT];  // heads of the chunk at or before the element
    GAgg run = ga_none();  // the open tail of the rounds so far
    uint64_t rstart = kNoHead;
    uint32_t heads = 0;
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        const uint64_t rb = cb + 64 * j;
        const uint64_t hm = hb[j] & le;  // the round's heads at or before this lane
        const uint32_t seg = hm ? top_bit(hm) : 0;
        if (AGG) {
            GAgg v = rb + lane < n ? GAgg{(int64_t)pay[j], pay[j], pay[j]} : ga_none();
            v = ga_seg_scan(v, lane - (int)seg);
            if (!hm) v = ga_comb(run, v);
            x[j] = v;
            run = GAgg{last_lane(v.sum), last_lane(v.mn), last_lane(v.mx)};
        }
        st[j] = hm ? rb + seg : rstart;
        if (hb[j]) rstart = rb + top_bit(hb[j]);
        hrank[j] = heads + (uint32_t)__popcll(hm);
        heads += (uint32_t)__popcll(hb[j]);
    }
    if (lane == 0) {
        L[w].tail = GCarry{run.sum, AGG == 2 ? (int64_t)run.mn : 0, AGG == 2 ? (int64_t)run.mx : 0,
                           rstart};
        L[w].heads = heads;
    }
    __syncthreads();
    // what comes in from the earlier tiles and the earlier waves of this one
    GCarry inc = carry[blockIdx.x];
    uint64_t row = row0;
#pragma unroll
    for (int v = 0; v < GA_WAVES - 1; v++) {
        if (v < w) {
            inc = gc_comb(inc, L[v].tail);
            row += L[v].heads;
        }
    }
    const GAgg ia{inc.sum, (MatVal)inc.mn, (MatVal)inc.mx};
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        const uint64_t rb = cb + 64 * j;
        const uint64_t gi = rb + lane;
        // the heads one element on: those of this round, then the first of
        // the next one; position n counts as a head
        uint64_t nx = j + 1 < GA_IPT ? hb[j + 1 < GA_IPT ? j + 1 : j] : (uint64_t)next_head;
        if (rb + 64 == n) nx = 1;
        uint64_t eb = (hb[j] >> 1) | (nx << 63);
        if (n > rb && n < rb + 64) eb |= 1ull << (n - rb - 1);
        if (!((eb >> lane) & 1) || gi >= n) continue;
        const uint64_t r = row + hrank[j] - 1;  // element 0 is a head: no row below 0
        if (r >= out_cap) continue;
        const bool far = st[j] == kNoHead;
        const uint64_t s = far ? inc.start : st[j];
        if (cols.key) {
            int64_t k = key[j];
            if (gsh != 0 && s < gi) k = ga_key(in + s);  // s <= gi < n
            st_col(cols.key + r, (MatVal)k);
        }
        if (cols.start) st_col(cols.start + r, (int64_t)s);
        if (cols.count) st_col(cols.count + r, (int64_t)(gi - s + 1));
        if (AGG) {
            const GAgg a = far ? ga_comb(ia, x[j]) : x[j];
            if (cols.sum) st_col(cols.sum + r, a.sum);
            if (AGG == 2 && cols.mn) st_col(cols.mn + r, a.mn);
            if (AGG == 2 && cols.mx) st_col(cols.mx + r, a.mx);
        }
    }
}

// materialize.hip's tile table with 0 bounds words (`bounds` is unused and
// equals `tot`) and, in tile_tab's extra bytes behind tot[0..1], the carry
// step's tables
struct GroupTab : TileTab {
    uint32_t nb;  // workgroups of the carry step
    GCarry *tail, *carry, *part, *pexcl;
};

static GroupTab group_tab(Workspace* ws, uint64_t n) {
    GroupTab g;
    const uint64_t ntiles = (n + GA_TILE - 1) / GA_TILE;
    g.nb = (uint32_t)((ntiles + GC_BLOCK - 1) / GC_BLOCK);
    const size_t pad = ((3 * ntiles) & 1) * 8;  // the GCarry tables 16-aligned
    static_cast<TileTab&>(g) = tile_tab(
        ws, "group_tab", ntiles, 0, pad + (2 * ntiles + 2 * (size_t)g.nb) * sizeof(GCarry));
    g.tail = (GCarry*)((char*)(g.tot + 2) + pad);
    g.carry = g.tail + g.ntiles;
    g.part = g.carry + g.ntiles;
    g.pexcl = g.part + g.nb;
    return g;
}

template <int AGG>
static void group_count_pass(Workspace* ws, const Tup* in, uint64_t n, uint32_t gsh,
                             const GroupTab& g, bool tails, hipStream_t st) {
    TraceScope ts(ws, "k_group_count", st);
    hipLaunchKernelGGL(k_group_count<AGG>, dim3((uint32_t)g.ntiles), dim3(GA_THREADS), 0, st, in,
                       n, gsh, g.cnt, tails ? g.tail : nullptr);
    SMJ_CHECK(hipGetLastError());
}

uint64_t group_aggregate(Workspace* ws, const Tup* in, uint64_t n, uint32_t group_shift,
                         void* key_out, int64_t* start_out, int64_t* count_out,
                         int64_t* sum_out, void* min_out, void* max_out, uint64_t out_cap,
                         hipStream_t st) {
    if (n == 0) return 0;
    const GroupCols cols{(MatVal*)key_out, start_out, count_out, sum_out, (MatVal*)min_out,
                         (MatVal*)max_out};
    const int agg = (cols.mn || cols.mx) ? 2 : cols.sum ? 1 : 0;
    const bool rows = out_cap && (agg || cols.key || cols.start || cols.count);
    const GroupTab g = group_tab(ws, n);
    if (rows && agg == 2) group_count_pass<2>(ws, in, n, group_shift, g, true, st);
    else if (rows && agg == 1) group_count_pass<1>(ws, in, n, group_shift, g, true, st);
    else group_count_pass<0>(ws, in, n, group_shift, g, rows, st);
    mat_scan(ws, g.cnt, g.ntiles, g.base, g.ibase, g.tot, st);
    if (rows) {
        {
            TraceScope ts(ws, "k_group_carry", st);
            hipLaunchKernelGGL(k_group_carry_part, dim3(g.nb), dim3(GC_BLOCK), 0, st, g.tail,
                               g.ntiles, g.part);
            SMJ_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_group_carry_pscan, dim3(1), dim3(GC_BLOCK), 0, st, g.part, g.nb,
                               g.pexcl);
            SMJ_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_group_carry_down, dim3(g.nb), dim3(GC_BLOCK), 0, st, g.tail,
                               g.ntiles, g.pexcl, g.carry);
            SMJ_CHECK(hipGetLastError());
        }
        // every tile is launched: those whose rows lie at out_cap and above
        // leave at once, so the launch needs no count on the host
        TraceScope ts(ws, "k_group_write", st);
        const dim3 grid((uint32_t)g.ntiles), block(GA_THREADS);
        if (agg == 2)
            hipLaunchKernelGGL(k_group_write<2>, grid, block, 0, st, in, n, group_shift, g.base,
                               g.carry, cols, out_cap);
        else if (agg == 1)
            hipLaunchKernelGGL(k_group_write<1>, grid, block, 0, st, in, n, group_shift, g.base,
                               g.carry, cols, out_cap);
        else
            hipLaunchKernelGGL(k_group_write<0>, grid, block, 0, st, in, n, group_shift, g.base,
                               g.carry, cols, out_cap);
        SMJ_CHECK(hipGetLastError());
    }
    uint64_t* h = (uint64_t*)ws->host_pinned("group_tot_h", 16);
    SMJ_CHECK(hipMemcpyAsync(h, g.tot, 16, hipMemcpyDeviceToHost, st));
    SMJ_CHECK(hipStreamSynchronize(st));
    return h[0];
}

void group_count(Workspace* ws, const Tup* in, uint64_t n, uint32_t group_shift,
                 unsigned long long* groups_dev, hipStream_t st) {
    if (n == 0) return;
    const GroupTab g = group_tab(ws, n);
    group_count_pass<0>(ws, in, n, group_shift, g, false, st);
    tile_total(ws, "k_group_total", g.cnt, g.ntiles, groups_dev, st);
}

}  // namespace smj
