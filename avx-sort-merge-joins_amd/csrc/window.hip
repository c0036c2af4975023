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
// The passes are groupagg.hip's, with its geometry (ga_common.hpp): a group
// spans any number of tiles and no workgroup waits for another.
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

constexpr uint32_t kNoOff = ~0u;  // a head offset in the chunk: in front of it

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

// the key level of an open tail: its last key head (kNoHead: none) and the
// key-only heads behind its last group head (in all of it when it has none)
struct KCarry {
    uint64_t kstart, dense;
};

__device__ __forceinline__ KCarry kc_none() { return KCarry{kNoHead, 0}; }

// a then b; cut: b has a group head, which closes a's count as it closes a's
// sum (gc_comb).  Field by field, as there
__device__ __forceinline__ KCarry kc_comb(const KCarry& a, const KCarry& b, bool cut) {
    KCarry r;
    r.kstart = b.kstart != kNoHead ? b.kstart : a.kstart;
    r.dense = cut ? b.dense : a.dense + b.dense;
    return r;
}

struct WWave {  // what a wave leaves for the others of its tile
    GCarry tail;
    KCarry k;
    uint32_t heads;
};

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

template <int AGG, bool RANKS>
__global__ void __launch_bounds__(GA_THREADS)
k_window_count(const Tup* __restrict__ in, uint64_t n, uint32_t gsh, uint64_t* __restrict__ cnt,
               GCarry* __restrict__ tail, KCarry* __restrict__ ktail) {
    __shared__ WWave L[GA_WAVES];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint64_t cb = (uint64_t)blockIdx.x * GA_TILE + (uint64_t)w * GA_CHUNK;
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT], kb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    if (RANKS) wn_key_heads(in, n, cb, key, kb);
    uint32_t heads = 0;
    uint64_t lstart = kNoHead, kstart = kNoHead;  // the chunk's last group head, key head
    uint64_t dense = 0;                           // key-only heads behind lstart
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        heads += (uint32_t)__popcll(hb[j]);
        if (hb[j]) lstart = cb + 64 * j + top_bit(hb[j]);
        if (RANKS) {
            const uint64_t ko = kb[j] & ~hb[j];
            if (hb[j]) dense = (uint64_t)__popcll(from_bit(ko, top_bit(hb[j])));
            else dense += (uint64_t)__popcll(ko);
            if (kb[j]) kstart = cb + 64 * j + top_bit(kb[j]);
        }
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
        if (RANKS) L[w].k = KCarry{kstart, dense};
        L[w].heads = heads;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        GCarry t = gc_none();
        KCarry k = kc_none();
        uint64_t h = 0;
#pragma unroll
        for (int v = 0; v < GA_WAVES; v++) {
            if (RANKS) k = kc_comb(k, L[v].k, L[v].tail.start != kNoHead);
            t = gc_comb(t, L[v].tail);
            h += L[v].heads;
        }
        cnt[blockIdx.x] = h;
        tail[blockIdx.x] = t;
        if (RANKS) ktail[blockIdx.x] = k;
    }
}

// ---- the carry step: groupagg.hip's, with the key level beside the tails

struct WCarry {
    GCarry g;
    KCarry k;
};

template <bool RANKS>
__device__ __forceinline__ WCarry wc_comb(const WCarry& a, const WCarry& b) {
    WCarry r;
    r.g = gc_comb(a.g, b.g);
    r.k = RANKS ? kc_comb(a.k, b.k, b.g.start != kNoHead) : kc_none();
    return r;
}

template <bool RANKS>
__device__ __forceinline__ WCarry wc_load(const GCarry* g, const KCarry* k, uint64_t i, bool in) {
    WCarry r;
    r.g = in ? g[i] : gc_none();
    r.k = RANKS && in ? k[i] : kc_none();
    return r;
}

template <bool RANKS>
__device__ __forceinline__ void wc_store(GCarry* g, KCarry* k, uint64_t i, const WCarry& v) {
    g[i] = v.g;
    if (RANKS) k[i] = v.k;
}

// gc_block_scan over both levels
template <bool RANKS>
__device__ __forceinline__ WCarry wc_block_scan(WCarry v, GCarry* wl, KCarry* wk, WCarry* total) {
    const int lane = lane_id(), wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        WCarry y;
        y.g.sum = sh_up(v.g.sum, o);
        y.g.mn = sh_up(v.g.mn, o);
        y.g.mx = sh_up(v.g.mx, o);
        y.g.start = (uint64_t)sh_up((int64_t)v.g.start, o);
        y.k = kc_none();
        if (RANKS) {
            y.k.kstart = (uint64_t)sh_up((int64_t)v.k.kstart, o);
            y.k.dense = (uint64_t)sh_up((int64_t)v.k.dense, o);
        }
        if (lane >= o) v = wc_comb<RANKS>(y, v);
    }
    if (lane == 63) {
        wl[wid] = v.g;
        if (RANKS) wk[wid] = v.k;
    }
    __syncthreads();
    WCarry p{gc_none(), kc_none()}, all{gc_none(), kc_none()};
#pragma unroll 1  // as in gc_block_scan
    for (int x = 0; x < (int)(GC_BLOCK / 64); x++) {
        if (x == wid) p = all;
        WCarry e;
        e.g = wl[x];
        e.k = RANKS ? wk[x] : kc_none();
        all = wc_comb<RANKS>(all, e);
    }
    *total = all;
    __syncthreads();  // wl and wk are free again
    return wc_comb<RANKS>(p, v);
}

// per GC_BLOCK tiles: their tails combined
template <bool RANKS>
__global__ void __launch_bounds__(GC_BLOCK)
k_window_carry_part(const GCarry* __restrict__ tail, const KCarry* __restrict__ ktail,
                    uint64_t ntiles, GCarry* __restrict__ part, KCarry* __restrict__ kpart) {
    __shared__ GCarry wl[GC_BLOCK / 64];
    __shared__ KCarry wk[GC_BLOCK / 64];
    const uint64_t t = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    WCarry all;
    wc_block_scan<RANKS>(wc_load<RANKS>(tail, ktail, t, t < ntiles), wl, wk, &all);
    if (threadIdx.x == 0) wc_store<RANKS>(part, kpart, blockIdx.x, all);
}

// pexcl[b] = the parts in front of workgroup b combined (one workgroup)
template <bool RANKS>
__global__ void __launch_bounds__(GC_BLOCK)
k_window_carry_pscan(const GCarry* __restrict__ part, const KCarry* __restrict__ kpart,
                     uint32_t nb, GCarry* __restrict__ pexcl, KCarry* __restrict__ kpexcl) {
    __shared__ GCarry wl[GC_BLOCK / 64];
    __shared__ KCarry wk[GC_BLOCK / 64];
    WCarry run{gc_none(), kc_none()};
    if (threadIdx.x == 0) wc_store<RANKS>(pexcl, kpexcl, 0, run);
    for (uint32_t r0 = 0; r0 < nb; r0 += GC_BLOCK) {
        const uint32_t b = r0 + threadIdx.x;
        WCarry all;
        const WCarry inc = wc_block_scan<RANKS>(wc_load<RANKS>(part, kpart, b, b < nb), wl, wk,
                                                &all);
        if (b + 1 < nb) wc_store<RANKS>(pexcl, kpexcl, b + 1, wc_comb<RANKS>(run, inc));
        run = wc_comb<RANKS>(run, all);
    }
}

// carry[t] = the tails of all tiles in front of tile t combined
template <bool RANKS>
__global__ void __launch_bounds__(GC_BLOCK)
k_window_carry_down(const GCarry* __restrict__ tail, const KCarry* __restrict__ ktail,
                    uint64_t ntiles, const GCarry* __restrict__ pexcl,
                    const KCarry* __restrict__ kpexcl, GCarry* __restrict__ carry,
                    KCarry* __restrict__ kcarry) {
    __shared__ GCarry wl[GC_BLOCK / 64];
    __shared__ KCarry wk[GC_BLOCK / 64];
    const uint64_t t = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    WCarry all;
    const WCarry inc =
        wc_block_scan<RANKS>(wc_load<RANKS>(tail, ktail, t, t < ntiles), wl, wk, &all);
    const WCarry front = wc_load<RANKS>(pexcl, kpexcl, blockIdx.x, true);
    if (t == 0) wc_store<RANKS>(carry, kcarry, 0, front);
    if (t + 1 < ntiles) wc_store<RANKS>(carry, kcarry, t + 1, wc_comb<RANKS>(front, inc));
}

template <int AGG, bool RANKS>
__global__ void __launch_bounds__(GA_THREADS)
k_window_write(const Tup* __restrict__ in, uint64_t n, uint32_t gsh,
               const uint64_t* __restrict__ base, const GCarry* __restrict__ carry,
               const KCarry* __restrict__ kcarry, WinCols cols) {
    __shared__ WWave L[GA_WAVES];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint64_t cb = (uint64_t)blockIdx.x * GA_TILE + (uint64_t)w * GA_CHUNK;
    const uint64_t le = lanemask_le();
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT], kb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    if (RANKS) wn_key_heads(in, n, cb, key, kb);

    // per element, as offsets in the chunk (kNoOff: in front of it)
    GAgg x[GA_IPT];          // aggregate from the element's group head, or the chunk's start
    uint32_t so[GA_IPT];     // its group head
    uint32_t ko[GA_IPT];     // its key head
    uint32_t hrank[GA_IPT];  // group heads of the chunk at or before it
    uint32_t dn[GA_IPT];     // key-only heads between its group head (the chunk's start) and it
    GAgg run = ga_none();    // the open tail of the rounds so far
    uint32_t rso = kNoOff, rko = kNoOff, heads = 0, drun = 0;
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        const uint64_t hm = hb[j] & le;  // the round's group heads at or before this lane
        const uint32_t seg = hm ? top_bit(hm) : 0;
        if (AGG) {
            GAgg v = cb + 64 * j + lane < n ? GAgg{(int64_t)pay[j], pay[j], pay[j]} : ga_none();
            v = ga_seg_scan(v, lane - (int)seg);
            if (!hm) v = ga_comb(run, v);
            x[j] = v;
            run = GAgg{last_lane(v.sum), last_lane(v.mn), last_lane(v.mx)};
        }
        so[j] = hm ? 64 * j + seg : rso;
        hrank[j] = heads + (uint32_t)__popcll(hm);
        if (RANKS) {
            const uint64_t km = kb[j] & le;
            ko[j] = km ? 64 * j + top_bit(km) : rko;
            if (kb[j]) rko = 64 * j + top_bit(kb[j]);
            const uint64_t only = kb[j] & ~hb[j];
            dn[j] = hm ? (uint32_t)__popcll(from_bit(only & le, seg))
                       : drun + (uint32_t)__popcll(only & le);
            if (hb[j]) drun = (uint32_t)__popcll(from_bit(only, top_bit(hb[j])));
            else drun += (uint32_t)__popcll(only);
        }
        if (hb[j]) rso = 64 * j + top_bit(hb[j]);
        heads += (uint32_t)__popcll(hb[j]);
    }
    if (lane == 0) {
        L[w].tail = GCarry{run.sum, AGG == 2 ? (int64_t)run.mn : 0, AGG == 2 ? (int64_t)run.mx : 0,
                           rso == kNoOff ? kNoHead : cb + rso};
        if (RANKS) L[w].k = KCarry{rko == kNoOff ? kNoHead : cb + rko, drun};
        L[w].heads = heads;
    }
    __syncthreads();
    // what comes in from the earlier tiles and the earlier waves of this one
    GCarry inc = carry[blockIdx.x];
    KCarry kinc = kc_none();
    if (RANKS) kinc = kcarry[blockIdx.x];
    uint64_t row = cols.group ? base[blockIdx.x] : 0;  // the group heads in front of the tile
#pragma unroll
    for (int v = 0; v < GA_WAVES - 1; v++) {
        if (v < w) {
            if (RANKS) kinc = kc_comb(kinc, L[v].k, L[v].tail.start != kNoHead);
            inc = gc_comb(inc, L[v].tail);
            row += L[v].heads;
        }
    }
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

// materialize.hip's tile table with 0 bounds words (`bounds` is unused and
// equals `tot`) and, in tile_tab's extra bytes behind tot[0..1], the carry
// step's tables, as groupagg.hip's GroupTab
struct WindowTab : TileTab {
    uint32_t nb;  // workgroups of the carry step
    GCarry *tail, *carry, *part, *pexcl;
    KCarry *ktail, *kcarry, *kpart, *kpexcl;  // null without RANKS
};

static WindowTab window_tab(Workspace* ws, uint64_t n, bool ranks) {
    WindowTab g;
    const uint64_t ntiles = (n + GA_TILE - 1) / GA_TILE;
    g.nb = (uint32_t)((ntiles + GC_BLOCK - 1) / GC_BLOCK);
    const size_t pad = ((3 * ntiles) & 1) * 8;  // the carry tables 16-aligned
    const size_t items = 2 * ntiles + 2 * (size_t)g.nb;
    static_cast<TileTab&>(g) = tile_tab(
        ws, "window_tab", ntiles, 0,
        pad + items * (sizeof(GCarry) + (ranks ? sizeof(KCarry) : 0)));
    g.tail = (GCarry*)((char*)(g.tot + 2) + pad);
    g.carry = g.tail + g.ntiles;
    g.part = g.carry + g.ntiles;
    g.pexcl = g.part + g.nb;
    g.ktail = ranks ? (KCarry*)(g.pexcl + g.nb) : nullptr;
    g.kcarry = ranks ? g.ktail + g.ntiles : nullptr;
    g.kpart = ranks ? g.kcarry + g.ntiles : nullptr;
    g.kpexcl = ranks ? g.kpart + g.nb : nullptr;
    return g;
}

template <int AGG, bool RANKS>
static void window_passes(Workspace* ws, const Tup* in, uint64_t n, uint32_t gsh,
                          const WinCols& cols, hipStream_t st) {
    const WindowTab g = window_tab(ws, n, RANKS);
    const dim3 grid((uint32_t)g.ntiles), block(GA_THREADS);
    {
        TraceScope ts(ws, "k_window_count", st);
        hipLaunchKernelGGL((k_window_count<AGG, RANKS>), grid, block, 0, st, in, n, gsh, g.cnt,
                           g.tail, g.ktail);
        SMJ_CHECK(hipGetLastError());
    }
    // the rows of the group table: only the group column reads them
    if (cols.group) mat_scan(ws, g.cnt, g.ntiles, g.base, g.ibase, g.tot, st);
    {
        TraceScope ts(ws, "k_window_carry", st);
        hipLaunchKernelGGL(k_window_carry_part<RANKS>, dim3(g.nb), dim3(GC_BLOCK), 0, st, g.tail,
                           g.ktail, g.ntiles, g.part, g.kpart);
        SMJ_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_window_carry_pscan<RANKS>, dim3(1), dim3(GC_BLOCK), 0, st, g.part,
                           g.kpart, g.nb, g.pexcl, g.kpexcl);
        SMJ_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_window_carry_down<RANKS>, dim3(g.nb), dim3(GC_BLOCK), 0, st, g.tail,
                           g.ktail, g.ntiles, g.pexcl, g.kpexcl, g.carry, g.kcarry);
        SMJ_CHECK(hipGetLastError());
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
    if (ranks) {
        if (agg == 2) window_passes<2, true>(ws, in, n, group_shift, cols, st);
        else if (agg == 1) window_passes<1, true>(ws, in, n, group_shift, cols, st);
        else window_passes<0, true>(ws, in, n, group_shift, cols, st);
    } else {
        if (agg == 2) window_passes<2, false>(ws, in, n, group_shift, cols, st);
        else if (agg == 1) window_passes<1, false>(ws, in, n, group_shift, cols, st);
        else window_passes<0, false>(ws, in, n, group_shift, cols, st);
    }
}

}  // namespace smj
