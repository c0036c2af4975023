// window.hip -- window functions over one sorted relation (smj.h
// smj_dev_window): one output row per tuple, PARTITION BY key >> group_shift
// ORDER BY key, ROWS UNBOUNDED PRECEDING: the tuple's group, its position in
// it, its rank and dense rank among the group's keys, and the running sum,
// minimum and maximum of the payloads up to it.  The library's own; the
// reference has joins only.
//
// Two levels of heads: element i is a group head when i == 0 or its group
// differs from that of element i - 1, and a key head when i == 0 or its key
// does; every group head is a key head.  With h(i) the last group head and
// p(i) the last key head at or before i, row = i - h, rank = p - h, dense rank
// = the key heads in (h, i], which are the key heads that are no group heads
// ("key-only" heads below).
//
// The passes are groupagg.hip's, with its geometry and its shared pieces
// (ga_common.hpp: ga_wave_tail, ga_walk, the carry step, tail_tab): a group
// spans any number of tiles and no workgroup waits for another.  Without RANKS
// the carry step is groupagg.hip's own (tail_carry); with RANKS it is the same
// kernels over WCarry, the two levels in parallel tables.
//   k_window_count one workgroup per tile: the tile's number of group heads
//                  and its open tail -- groupagg.hip's GCarry, and with RANKS
//                  the key level (KCarry): the position of its last key head
//                  and the number of key-only heads behind its last group
//                  head (of the whole tile when it has none);
//   k_mat_scan     materialize.hip's, over the head counts: the group heads in
//                  front of every tile (only when the group column is asked
//                  for; its total is not read);
//   k_window_carry the segmented scan of the tails over the tiles, both
//                  levels in one scan: a group head in b closes a's sum and
//                  a's count of key-only heads alike;
//   k_window_write one workgroup per tile: reads the tile again and writes
//                  every column at every element.  Positions and ranks come
//                  from top_bit / popcount of the rounds' two head ballots;
//                  only sum, minimum and maximum go through ga_seg_scan.  An
//                  element whose group head lies in front of its chunk adds
//                  what came in from the earlier waves and the tile's carry.
// Both tile kernels are templates of the aggregate level (0: none, 1: sum, 2:
// minimum and maximum too) and of RANKS (rank or dense rank asked for): a call
// for row and sum pays neither registers nor tables for the key level.
// Stream-ordered: a row per tuple needs no count on the host.
#include "smj_common.hpp"
#include "smj_internal.hpp"
#include "mat_common.hpp"
#include "ga_common.hpp"

namespace smj {

uint32_t window_tile() { return GA_TILE; }

// the output columns (each may be null)
struct WinCols {
    int64_t* group;
    int64_t* row;
    int64_t* rank;
    int64_t* dense;
    int64_t* sum;
    MatVal* mn;
    MatVal* mx;
};

// the key level of an open tail is ga_common.hpp's KCarry
__device__ __forceinline__ KCarry kc_none() { return KCarry{kNoHead, 0}; }

// a then b; cut: b has a group head, which closes a's count as it closes a's
// sum (gc_comb).  Field by field, as there
__device__ __forceinline__ KCarry kc_comb(const KCarry& a, const KCarry& b, bool cut) {
    KCarry r;
    r.kstart = b.kstart != kNoHead ? b.kstart : a.kstart;
    r.dense = cut ? b.dense : a.dense + b.dense;
    return r;
}

// per round the ballot of the key heads of the wave's chunk (ga_load's head
// ballots with the whole key for the group)
__device__ __forceinline__ void wn_key_heads(const Tup* __restrict__ in, uint64_t n, uint64_t cb,
                                             const int64_t (&key)[GA_IPT],
                                             uint64_t (&kb)[GA_IPT]) {
    const int lane = lane_id();
    int64_t last = 0;
    if (cb > 0 && cb < n) last = ga_key(in + cb - 1);
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        const uint64_t gi = cb + 64 * j + lane;
        int64_t pk = dpp<kDppWaveShr1, 0xf>(key[j]);
        if (lane == 0) pk = last;
        kb[j] = __ballot(gi < n && (gi == 0 || key[j] != pk));
        last = last_lane(key[j]);
    }
}

// the bits of m at and above bit b
__device__ __forceinline__ uint64_t from_bit(uint64_t m, uint32_t b) { return m & (~0ull << b); }

// groupagg.hip's count pass; with RANKS the key level beside it
template <int AGG, bool RANKS>
__global__ void __launch_bounds__(GA_THREADS)
k_window_count(const Tup* __restrict__ in, uint64_t n, uint32_t gsh, uint64_t* __restrict__ cnt,
               GCarry* __restrict__ tail, KCarry* __restrict__ ktail) {
    __shared__ GWave L[GA_WAVES];
    __shared__ KCarry LK[RANKS ? GA_WAVES : 1];
    const int w = threadIdx.x >> 6;
    const uint64_t cb = (uint64_t)blockIdx.x * GA_TILE + (uint64_t)w * GA_CHUNK;
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    if (RANKS) {
        uint64_t kb[GA_IPT];
        wn_key_heads(in, n, cb, key, kb);
        uint32_t kso = kNoOff;  // the chunk's last key head
        uint32_t dense = 0;     // key-only heads behind its last group head
#pragma unroll
        for (int j = 0; j < GA_IPT; j++) {
            const uint64_t ko = kb[j] & ~hb[j];
            if (hb[j]) dense = (uint32_t)__popcll(from_bit(ko, top_bit(hb[j])));
            else dense += (uint32_t)__popcll(ko);
            if (kb[j]) kso = 64 * j + top_bit(kb[j]);
        }
        if (lane_id() == 0) LK[w] = KCarry{kso == kNoOff ? kNoHead : cb + kso, dense};
    }
    ga_wave_tail<AGG>(n, cb, pay, hb, &L[w]);
    __syncthreads();
    if (threadIdx.x == 0) {
        // (written out: through a shared fold of the waves, k_group_count<0> took 27
        // VGPRs for 26 and k_window_count<0, true> 34 for 32 at 8-byte tuples)
        GCarry t = gc_none();
        KCarry k = kc_none();
        uint64_t h = 0;
#pragma unroll
        for (int v = 0; v < GA_WAVES; v++) {
            if (RANKS) k = kc_comb(k, LK[v], L[v].tail.start != kNoHead);
            t = gc_comb(t, L[v].tail);
            h += L[v].heads;
        }
        cnt[blockIdx.x] = h;
        tail[blockIdx.x] = t;
        if (RANKS) ktail[blockIdx.x] = k;
    }
}

// ---- the carry step with RANKS: both levels in one scan (without, the
// tails alone: ga_common.hpp's tail_carry, groupagg.hip's kernels)

struct WCarry {
    GCarry g;
    KCarry k;
};

struct WCarryOps {
    typedef WCarry T;
    struct Shared {
        GCarry g[GC_BLOCK / 64];
        KCarry k[GC_BLOCK / 64];
        __device__ __forceinline__ void put(int i, const T& v) { g[i] = v.g; k[i] = v.k; }
        __device__ __forceinline__ T get(int i) const { return WCarry{g[i], k[i]}; }
    };
    static __device__ __forceinline__ T none() { return WCarry{gc_none(), kc_none()}; }
    static __device__ __forceinline__ T comb(const T& a, const T& b) {
        WCarry r;
        r.g = gc_comb(a.g, b.g);
        r.k = kc_comb(a.k, b.k, b.g.start != kNoHead);
        return r;
    }
    static __device__ __forceinline__ T up(const T& v, int o) {
        WCarry y;
        y.g = GCarryOps::up(v.g, o);
        y.k.kstart = (uint64_t)sh_up((int64_t)v.k.kstart, o);
        y.k.dense = (uint64_t)sh_up((int64_t)v.k.dense, o);
        return y;
    }
};

struct WCarryTable {  // the two levels in parallel tables
    GCarry* g;
    KCarry* k;
    __device__ __forceinline__ WCarry load(uint64_t i) const { return WCarry{g[i], k[i]}; }
    __device__ __forceinline__ void store(uint64_t i, const WCarry& v) const {
        g[i] = v.g;
        k[i] = v.k;
    }
};

template <int AGG, bool RANKS>
__global__ void __launch_bounds__(GA_THREADS)
k_window_write(const Tup* __restrict__ in, uint64_t n, uint32_t gsh,
               const uint64_t* __restrict__ base, const GCarry* __restrict__ carry,
               const KCarry* __restrict__ kcarry, WinCols cols) {
    __shared__ GWave L[GA_WAVES];
    __shared__ KCarry LK[RANKS ? GA_WAVES : 1];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint64_t cb = (uint64_t)blockIdx.x * GA_TILE + (uint64_t)w * GA_CHUNK;
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT], kb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    if (RANKS) wn_key_heads(in, n, cb, key, kb);

    // per element (ga_walk), and as offsets in the chunk (kNoOff: in front of it)
    GAgg x[GA_IPT];
    uint32_t so[GA_IPT], hrank[GA_IPT];
    uint32_t ko[GA_IPT];  // its key head
    uint32_t dn[GA_IPT];  // key-only heads between its group head (the chunk's start) and it
    const GWave mine = ga_walk<AGG>(n, cb, pay, hb, x, so, hrank);
    if (lane == 0) L[w] = mine;
    if (RANKS) {
        const uint64_t le = lanemask_le();
        uint32_t rko = kNoOff, drun = 0;
#pragma unroll
        for (int j = 0; j < GA_IPT; j++) {
            const uint64_t hm = hb[j] & le, km = kb[j] & le;
            ko[j] = km ? 64 * j + top_bit(km) : rko;
            if (kb[j]) rko = 64 * j + top_bit(kb[j]);
            const uint64_t only = kb[j] & ~hb[j];
            dn[j] = hm ? (uint32_t)__popcll(from_bit(only & le, top_bit(hm)))
                       : drun + (uint32_t)__popcll(only & le);
            if (hb[j]) drun = (uint32_t)__popcll(from_bit(only, top_bit(hb[j])));
            else drun += (uint32_t)__popcll(only);
        }
        if (lane == 0) LK[w] = KCarry{rko == kNoOff ? kNoHead : cb + rko, drun};
    }
    __syncthreads();
    // what comes in from the earlier tiles and the earlier waves of this one
    GCarry inc = carry[blockIdx.x];
    uint64_t row = cols.group ? base[blockIdx.x] : 0;  // the group heads in front of the tile
    KCarry kinc = kc_none();
    if (RANKS) {
        kinc = kcarry[blockIdx.x];
#pragma unroll
        for (int v = 0; v < GA_WAVES - 1; v++)
            if (v < w) kinc = kc_comb(kinc, LK[v], L[v].tail.start != kNoHead);
    }
    ga_incoming(L, w, inc, row);
    const GAgg ia{inc.sum, (MatVal)inc.mn, (MatVal)inc.mx};
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        const uint64_t gi = cb + 64 * j + lane;
        if (gi >= n) continue;
        // element 0 is a head: an element with its head in front of the chunk
        // has earlier waves or tiles, and inc holds that head
        const bool far = so[j] == kNoOff;
        const uint64_t h = far ? inc.start : cb + so[j];
        if (cols.group) st_col(cols.group + gi, (int64_t)(row + hrank[j] - 1));
        if (cols.row) st_col(cols.row + gi, (int64_t)(gi - h));
        if (RANKS) {
            const uint64_t p = ko[j] == kNoOff ? kinc.kstart : cb + ko[j];
            if (cols.rank) st_col(cols.rank + gi, (int64_t)(p - h));
            if (cols.dense) st_col(cols.dense + gi, (int64_t)((far ? kinc.dense : 0) + dn[j]));
        }
        if (AGG) {
            const GAgg a = far ? ga_comb(ia, x[j]) : x[j];
            if (cols.sum) st_col(cols.sum + gi, a.sum);
            if (AGG == 2 && cols.mn) st_col(cols.mn + gi, a.mn);
            if (AGG == 2 && cols.mx) st_col(cols.mx + gi, a.mx);
        }
    }
}

template <int AGG, bool RANKS>
static void window_passes(Workspace* ws, const Tup* in, uint64_t n, uint32_t gsh,
                          const WinCols& cols, hipStream_t st) {
    const TailTab g = tail_tab(ws, "window_tab", n, RANKS);
    const dim3 grid((uint32_t)g.ntiles), block(GA_THREADS);
    {
        TraceScope ts(ws, "k_window_count", st);
        hipLaunchKernelGGL((k_window_count<AGG, RANKS>), grid, block, 0, st, in, n, gsh, g.cnt,
                           g.tail, g.ktail);
        SMJ_CHECK(hipGetLastError());
    }
    // the rows of the group table: only the group column reads them
    if (cols.group) mat_scan(ws, g.cnt, g.ntiles, g.base, g.ibase, g.tot, st);
    if constexpr (RANKS) {
        typedef WCarryTable Tab;
        carry_scan<WCarryOps>(ws, "k_window_carry", Tab{g.tail, g.ktail}, g.ntiles,
                              Tab{g.part, g.kpart}, Tab{g.pexcl, g.kpexcl},
                              Tab{g.carry, g.kcarry}, st);
    } else {
        tail_carry(ws, "k_window_carry", g, st);
    }
    TraceScope ts(ws, "k_window_write", st);
    hipLaunchKernelGGL((k_window_write<AGG, RANKS>), grid, block, 0, st, in, n, gsh, g.base,
                       g.carry, g.kcarry, cols);
    SMJ_CHECK(hipGetLastError());
}

void window(Workspace* ws, const Tup* in, uint64_t n, uint32_t group_shift, int64_t* group_out,
            int64_t* row_out, int64_t* rank_out, int64_t* dense_rank_out, int64_t* sum_out,
            void* min_out, void* max_out, hipStream_t st) {
    const WinCols cols{group_out, row_out, rank_out, dense_rank_out, sum_out, (MatVal*)min_out,
                       (MatVal*)max_out};
    const int agg = (cols.mn || cols.mx) ? 2 : cols.sum ? 1 : 0;
    const bool ranks = cols.rank || cols.dense;
    if (n == 0 || !(agg || ranks || cols.group || cols.row)) return;
    with_agg(agg, [&](auto A) {
        with_flag(ranks, [&](auto R) {
            window_passes<decltype(A)::value, decltype(R)::value>(ws, in, n, group_shift, cols,
                                                                  st);
        });
    });
}

}  // namespace smj
