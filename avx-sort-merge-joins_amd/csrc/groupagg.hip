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
// What window.hip and frame.hip use as well lies in ga_common.hpp: the
// geometry, GAgg and GCarry, the lane moves, ga_load, ga_seg_scan, the count
// pass's wave (ga_wave_tail), the write pass's chunk walk (ga_walk,
// ga_incoming), the carry step (k_carry_*, of which tail_carry() here is the
// GCarry instance, window.hip's too) and the table (tail_tab).
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

// AGG 0: the tails' head positions alone (tail may be null: the count form),
// 1: with their sums, 2: with minimum and maximum as well (what nobody asks
// for is not computed: the scans are what the passes spend their time on).
template <int AGG>
__global__ void __launch_bounds__(GA_THREADS)
k_group_count(const Tup* __restrict__ in, uint64_t n, uint32_t gsh, uint64_t* __restrict__ cnt,
              GCarry* __restrict__ tail) {
    __shared__ GWave L[GA_WAVES];
    const int w = threadIdx.x >> 6;
    const uint64_t cb = (uint64_t)blockIdx.x * GA_TILE + (uint64_t)w * GA_CHUNK;
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    ga_wave_tail<AGG>(n, cb, pay, hb, &L[w]);
    __syncthreads();
    if (threadIdx.x == 0) {
        // (written out: through a shared fold of the waves, k_group_count<0> took 27
        // VGPRs for 26 and k_window_count<0, true> 34 for 32 at 8-byte tuples)
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
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    // is the element behind the chunk a head (the relation's end counts)
    const uint64_t ce = cb + GA_CHUNK;
    bool next_head = ce == n;
    if (ce < n) next_head = (ga_key(in + ce) >> gsh) != (ga_key(in + ce - 1) >> gsh);

    GAgg x[GA_IPT];
    uint32_t so[GA_IPT], hrank[GA_IPT];
    const GWave mine = ga_walk<AGG>(n, cb, pay, hb, x, so, hrank);
    if (lane == 0) L[w] = mine;
    __syncthreads();
    GCarry inc = carry[blockIdx.x];
    uint64_t row = row0;
    ga_incoming(L, w, inc, row);
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
        const bool far = so[j] == kNoOff;
        const uint64_t s = far ? inc.start : cb + so[j];
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

void tail_carry(Workspace* ws, const char* name, const TailTab& g, hipStream_t st) {
    typedef CarryTable<GCarry> Tab;
    carry_scan<GCarryOps>(ws, name, Tab{g.tail}, g.ntiles, Tab{g.part}, Tab{g.pexcl},
                          Tab{g.carry}, st);
}

template <int AGG>
static void group_count_pass(Workspace* ws, const Tup* in, uint64_t n, uint32_t gsh,
                             const TailTab& g, bool tails, hipStream_t st) {
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
    const TailTab g = tail_tab(ws, "group_tab", n, false);
    // without rows, the count form
    with_agg(rows ? agg : 0, [&](auto A) {
        group_count_pass<decltype(A)::value>(ws, in, n, group_shift, g, rows, st);
    });
    mat_scan(ws, g.cnt, g.ntiles, g.base, g.ibase, g.tot, st);
    if (rows) {
        tail_carry(ws, "k_group_carry", g, st);
        // every tile is launched: those whose rows lie at out_cap and above
        // leave at once, so the launch needs no count on the host
        TraceScope ts(ws, "k_group_write", st);
        with_agg(agg, [&](auto A) {
            hipLaunchKernelGGL(k_group_write<decltype(A)::value>, dim3((uint32_t)g.ntiles),
                               dim3(GA_THREADS), 0, st, in, n, group_shift, g.base, g.carry, cols,
                               out_cap);
        });
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
    const TailTab g = tail_tab(ws, "group_tab", n, false);
    group_count_pass<0>(ws, in, n, group_shift, g, false, st);
    tile_total(ws, "k_group_total", g.cnt, g.ntiles, groups_dev, st);
}

}  // namespace smj
