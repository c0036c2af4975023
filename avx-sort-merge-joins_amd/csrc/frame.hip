// frame.hip -- sliding window frames over one sorted relation (smj.h
// smj_dev_window_frame): one output row per tuple, PARTITION BY key >>
// group_shift ORDER BY key, with the frame ROWS or RANGE BETWEEN lo AND hi
// around the tuple: where the frame starts, how many tuples it holds, the sum,
// minimum and maximum of their payloads and the payloads of its first and last
// tuple.  The library's own; the reference has joins only.
//
// With h(i) the last group head at or before i and e(i) the last element of
// i's group, the frame of i is the positions [a, b] of [h, e] with
//   ROWS   i + lo <= j <= i + hi                      (saturating),
//   RANGE  key[i] + lo <= key[j] <= key[i] + hi       (bandjoin.hip's sat_add).
// An aggregate over an arbitrary [a, b] costs a bounded number of loads,
// whatever the frame's width:
//   sum      P(b) - P(a) + payload[a], P(j) = the exclusive scan of the tile
//            sums at j's tile plus the inclusive prefix sum inside the tile;
//   min/max  a and b in one aligned block of FR_BLOCK elements: the elements
//            themselves; otherwise the suffix of a's block at a, the prefix of
//            b's block at b, and between them: in one tile the block
//            aggregates (at most 14), in two tiles the suffix over a's tile's
//            blocks behind a's, the prefix over b's tile's blocks in front of
//            b's, and one pair of entries of a sparse table over the whole
//            tiles between (level k entry t = tiles [t, t + 2^k)).
// The passes, over ga_common.hpp's tiles:
//   k_frame_build one workgroup per tile, only when sum, min or max is asked
//                 for: the in-tile prefix sums, the prefix and suffix extremes
//                 inside the blocks, the block aggregates with their prefix
//                 and suffix inside the tile, the tile's aggregate and its
//                 first and last group head;
//   k_frame_scan  small kernels over the tile tables: one scan over the tiles
//                 carries the sums and the last head forward and, on the
//                 mirrored index, the first head backward (sum, max and min
//                 commute, so one instance of ga_common.hpp's carry step does
//                 all three); then the sparse table, a launch a level.  A call
//                 without aggregates has no build pass, and the step's first
//                 kernel takes the tiles' heads from the keys itself;
//   k_frame_write one workgroup per tile: h and e from the tile's head
//                 ballots and the two carried tables, the frame's ends, the
//                 look-ups above and the columns.
// RANGE ends are searched per row, galloping from the row itself towards the
// end (backward for a bound at or below the row's key, forward above it) and
// clamped to [h, e]: O(log distance) probes.  The tile's keys are staged in
// LDS; one look at the tile's last (first) key of the group says whether the
// end lies inside the tile, where the search runs on 32-bit offsets into the
// staged keys, or outside, where one look at the group's last (first) key
// answers a band that reaches the group's end and the relation is searched
// otherwise.  The band join's staged R window per tile would need the bounds
// of the tile's first and last row first and still leaves far ends to the
// unstaged search; a frame's ends start from a known place (the row), which a
// join's do not.
// Stream-ordered: a row per tuple needs no count on the host.
#include "smj_common.hpp"
#include "smj_internal.hpp"
#include "mat_common.hpp"
#include "ga_common.hpp"

namespace smj {

constexpr uint32_t FR_BLOCK = 64;                  // the inner aligned block: a wave round
constexpr uint32_t FR_WORDS = GA_TILE / FR_BLOCK;  // blocks (head ballots) of a tile
static_assert(GA_TILE % FR_BLOCK == 0 && FR_WORDS <= 64, "blocks tile the tile");

uint32_t frame_tile() { return GA_TILE; }
uint32_t frame_block() { return FR_BLOCK; }

// the output columns (each may be null)
struct FrameCols {
    int64_t *start, *count, *sum;
    MatVal *mn, *mx, *first, *last;
};

// what the scan step carries over the tiles: the sum and the last head of the
// tiles in front (-1: none), the first head of the tiles behind (kNoHead)
struct FCarry {
    int64_t sum, last;
    uint64_t first;
};

// the workspace's tables of one call; those no asked column needs are null
struct FrameTab {
    uint64_t ntiles;
    uint32_t levels;  // of the sparse table, level 0 being the tiles themselves
    int64_t *tsum, *texcl;      // per tile: its sum, the sum of the tiles in front
    int64_t *tlast, *hprev;     // its last head (-1), the last head in front of it
    uint64_t *tfirst, *hnext;   // its first head (kNoHead), the first behind it (n)
    FCarry *part, *pexcl;       // per scan workgroup
    int64_t* pre;               // per element: the inclusive prefix sum in its tile
    MatVal *pmn, *smn, *pmx, *smx;  // per element: prefix and suffix in its block
    MatVal *bmn, *bmx;          // per block
    MatVal *bpmn, *bsmn, *bpmx, *bsmx;  // per block: prefix and suffix over its tile's blocks
    MatVal *spmn, *spmx;        // levels x ntiles
};

__device__ __forceinline__ int64_t sh_rev(int64_t v) {
    return (int64_t)__shfl((unsigned long long)v, 63 - lane_id(), 64);
}
__device__ __forceinline__ int32_t sh_rev(int32_t v) { return __shfl(v, 63 - lane_id(), 64); }

__device__ __forceinline__ uint32_t low_bit(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }

// ---- the build pass

struct FWave {  // what a wave leaves for its tile
    int64_t sum, last;
    uint64_t first;
    MatVal mn, mx;
};

struct FBuildLDS {
    FWave w[GA_WAVES];
    MatVal bmn[FR_WORDS], bmx[FR_WORDS];  // the blocks' extremes
};

// one tile; AGG 0: its first and last head and nothing else, 1: the sums too,
// 2: the extremes too (window.hip's levels)
template <int AGG>
__device__ __forceinline__ void frame_build_tile(const Tup* __restrict__ in, uint64_t n,
                                                 uint32_t gsh, const FrameTab& g, FBuildLDS& L) {
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint64_t cb = (uint64_t)blockIdx.x * GA_TILE + (uint64_t)w * GA_CHUNK;
    int64_t key[GA_IPT];
    MatVal pay[GA_IPT];
    uint64_t hb[GA_IPT];
    ga_load<AGG != 0>(in, n, cb, gsh, key, pay, hb);
    uint64_t first = kNoHead;
    int64_t last = -1;
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        if (hb[j]) {
            if (first == kNoHead) first = cb + 64 * j + low_bit(hb[j]);
            last = (int64_t)(cb + 64 * j + top_bit(hb[j]));
        }
    }
    int64_t pre[GA_IPT];  // the prefix sum inside the chunk
    GAgg run = ga_none();
    if (AGG) {
#pragma unroll
        for (int j = 0; j < GA_IPT; j++) {
            const uint64_t gi = cb + 64 * j + lane;
            const bool in_rel = gi < n;
            const GAgg v = in_rel ? ga_one(pay[j]) : ga_none();
            const GAgg p = ga_seg_scan(v, lane);  // the prefix over the block
            pre[j] = (int64_t)((uint64_t)run.sum + (uint64_t)p.sum);
            const GAgg all{last_lane(p.sum), last_lane(p.mn), last_lane(p.mx)};
            if (AGG == 2) {
                // the suffix: the prefix of the lanes in reverse order
                const GAgg r = ga_seg_scan(GAgg{0, sh_rev(v.mn), sh_rev(v.mx)}, lane);
                const MatVal smn = sh_rev(r.mn), smx = sh_rev(r.mx);
                if (in_rel && g.pmn) {
                    g.pmn[gi] = p.mn;
                    g.smn[gi] = smn;
                }
                if (in_rel && g.pmx) {
                    g.pmx[gi] = p.mx;
                    g.smx[gi] = smx;
                }
                if (lane == 0) {
                    L.bmn[w * GA_IPT + j] = all.mn;
                    L.bmx[w * GA_IPT + j] = all.mx;
                }
            }
            run = ga_comb(run, all);
        }
    }
    if (lane == 0) L.w[w] = FWave{run.sum, last, first, run.mn, run.mx};
    __syncthreads();
    if (AGG && g.pre) {
        uint64_t front = 0;  // the waves in front
#pragma unroll
        for (int v = 0; v < GA_WAVES - 1; v++)
            if (v < w) front += (uint64_t)L.w[v].sum;
#pragma unroll
        for (int j = 0; j < GA_IPT; j++) {
            const uint64_t gi = cb + 64 * j + lane;
            if (gi < n) g.pre[gi] = (int64_t)(front + (uint64_t)pre[j]);
        }
    }
    if (AGG == 2 && threadIdx.x < FR_WORDS) {
        // block x: itself, and with the blocks of the tile in front of and behind it
        // (blocks behind the relation hold ga_none's values)
        const int x = threadIdx.x;
        const uint64_t q = (uint64_t)blockIdx.x * FR_WORDS + x;
        if (q * FR_BLOCK < n) {
            MatVal pmn = L.bmn[x], pmx = L.bmx[x], smn = pmn, smx = pmx;
            if (g.bmn) g.bmn[q] = pmn;
            if (g.bmx) g.bmx[q] = pmx;
            for (int y = 0; y < x; y++) {
                pmn = vmin(pmn, L.bmn[y]);
                pmx = vmax(pmx, L.bmx[y]);
            }
            for (int y = x + 1; y < (int)FR_WORDS; y++) {
                smn = vmin(smn, L.bmn[y]);
                smx = vmax(smx, L.bmx[y]);
            }
            if (g.bmn) {
                g.bpmn[q] = pmn;
                g.bsmn[q] = smn;
            }
            if (g.bmx) {
                g.bpmx[q] = pmx;
                g.bsmx[q] = smx;
            }
        }
    }
    if (threadIdx.x == 0) {
        GAgg a = ga_none();
        uint64_t f = kNoHead;
        int64_t l = -1;
#pragma unroll
        for (int v = 0; v < GA_WAVES; v++) {
            a = ga_comb(a, GAgg{L.w[v].sum, L.w[v].mn, L.w[v].mx});
            if (f == kNoHead) f = L.w[v].first;
            if (L.w[v].last >= 0) l = L.w[v].last;
        }
        g.tfirst[blockIdx.x] = f;
        g.tlast[blockIdx.x] = l;
        if (AGG && g.tsum) g.tsum[blockIdx.x] = a.sum;
        if (AGG == 2 && g.spmn) g.spmn[blockIdx.x] = a.mn;
        if (AGG == 2 && g.spmx) g.spmx[blockIdx.x] = a.mx;
    }
}

template <int AGG>
__global__ void __launch_bounds__(GA_THREADS)
k_frame_build(const Tup* __restrict__ in, uint64_t n, uint32_t gsh, FrameTab g) {
    __shared__ FBuildLDS L;
    frame_build_tile<AGG>(in, n, gsh, g, L);
}

// ---- the scan step

// the heads of the tiles when no build pass has run: the keys alone
__global__ void __launch_bounds__(GA_THREADS)
k_frame_scan_heads(const Tup* __restrict__ in, uint64_t n, uint32_t gsh, FrameTab g) {
    __shared__ FBuildLDS L;
    frame_build_tile<0>(in, n, gsh, g, L);
}

struct FCarryOps {
    typedef FCarry T;
    typedef CarryShared<FCarry> Shared;
    static __device__ __forceinline__ T none() { return FCarry{0, -1, kNoHead}; }
    static __device__ __forceinline__ T comb(const T& a, const T& b) {
        return FCarry{(int64_t)((uint64_t)a.sum + (uint64_t)b.sum), vmax(a.last, b.last),
                      vmin(a.first, b.first)};
    }
    static __device__ __forceinline__ T up(const T& v, int o) {
        T y;
        y.sum = sh_up(v.sum, o);
        y.last = sh_up(v.last, o);
        y.first = (uint64_t)sh_up((int64_t)v.first, o);
        return y;
    }
};

// item x of the scan: tile x of the forward fields, tile ntiles - 1 - x of the
// backward one
struct FTiles {
    const int64_t *tsum, *tlast;
    const uint64_t* tfirst;
    uint64_t ntiles;
    __device__ __forceinline__ FCarry load(uint64_t x) const {
        return FCarry{tsum ? tsum[x] : 0, tlast[x], tfirst[ntiles - 1 - x]};
    }
};

// what lies in front of item x into the tables of its tiles
struct FFronts {
    int64_t *texcl, *hprev;
    uint64_t* hnext;
    uint64_t ntiles, n;
    __device__ __forceinline__ void store(uint64_t x, const FCarry& v) const {
        if (texcl) texcl[x] = v.sum;
        hprev[x] = v.last;
        hnext[ntiles - 1 - x] = v.first == kNoHead ? n : v.first;
    }
};

// level k of the sparse table from level k - 1: entry t = tiles [t, t + 2^k)
// (entries whose range leaves the relation are never read)
__global__ void __launch_bounds__(256) k_frame_scan_sparse(FrameTab g, uint32_t k) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= g.ntiles) return;
    const uint64_t half = 1ull << (k - 1);
    const uint64_t o = t + half < g.ntiles ? t + half : t;
    const uint64_t src = (uint64_t)(k - 1) * g.ntiles, dst = (uint64_t)k * g.ntiles;
    if (g.spmn) g.spmn[dst + t] = vmin(g.spmn[src + t], g.spmn[src + o]);
    if (g.spmx) g.spmx[dst + t] = vmax(g.spmx[src + t], g.spmx[src + o]);
}

// ---- the write pass

// The searches of a RANGE end are mat_common.hpp's, on 32-bit offsets into the
// tile's staged keys, where most ends lie, and on positions in the relation.

// key_gallop with one search behind the loop (written out: through key_gallop
// the RANGE write kernels took 44 VGPRs for 38, and key_gallop in this form
// changed the registers of the join-output kernels)
template <bool UPPER, class I, class K>
__device__ __forceinline__ I fr_gallop(K key, I lo, I hi, int64_t k) {
    I step = 1;
    while (hi - lo >= step && key_before<UPPER>(key(lo + step - 1), k)) {
        lo += step;
        step <<= 1;
    }
    return key_search<UPPER, I>(key, lo, hi - lo >= step ? lo + step - 1 : hi, k);
}

// The first position of [from, to) whose key is not before k (to: none), for a
// row of the tile [tb, te) with tb < from <= te: inside the tile when its last
// key there says so, else behind it, where the group's last key may already
// answer (a band that reaches the group's end: a hot key costs two probes)
template <bool UPPER>
__device__ __forceinline__ uint64_t frame_end_fwd(const Tup* __restrict__ in, const int64_t* lkey,
                                                  uint64_t tb, uint64_t te, uint64_t from,
                                                  uint64_t to, int64_t k) {
    const uint64_t tl = to < te ? to : te;
    if (from < tl && !key_before<UPPER>(lkey[tl - 1 - tb], k))
        return tb + fr_gallop<UPPER>(LdsKey{lkey}, (uint32_t)(from - tb), (uint32_t)(tl - tb), k);
    if (to <= te) return to;
    if (key_before<UPPER>(ga_key(in + to - 1), k)) return to;
    return fr_gallop<UPPER>(TupKey{in}, te, to, k);
}

// The first position of [lo, hi) whose key is not before k (hi: none, the
// row itself), for the row hi of the tile that begins at tb <= hi, backward
template <bool UPPER>
__device__ __forceinline__ uint64_t frame_end_back(const Tup* __restrict__ in, const int64_t* lkey,
                                                   uint64_t tb, uint64_t lo, uint64_t hi,
                                                   int64_t k) {
    const uint64_t fl = lo > tb ? lo : tb;
    if (fl < hi && key_before<UPPER>(lkey[fl - tb], k))
        return tb + key_gallop_back<UPPER, uint32_t>(LdsKey{lkey}, (uint32_t)(fl + 1 - tb),
                                                     (uint32_t)(hi - tb), k);
    if (lo >= tb) return fl;
    if (!key_before<UPPER>(ga_key(in + lo), k)) return lo;
    return key_gallop_back<UPPER>(TupKey{in}, lo, tb, k);
}

template <int AGG, bool RANGE>
__global__ void __launch_bounds__(GA_THREADS)
k_frame_write(const Tup* __restrict__ in, uint64_t n, uint32_t gsh, int64_t lo, int64_t hi,
              FrameTab g, FrameCols cols) {
    __shared__ uint64_t Lhb[FR_WORDS];   // the blocks' head ballots
    __shared__ int64_t Lprev[FR_WORDS];  // the last head in front of each block
    __shared__ int64_t Lnext[FR_WORDS];  // the first head behind it (n: none)
    __shared__ int64_t Lkey[RANGE ? GA_TILE : 1];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint64_t tb = (uint64_t)blockIdx.x * GA_TILE;
    const uint64_t cb = tb + (uint64_t)w * GA_CHUNK;
    {
        int64_t key[GA_IPT];
        MatVal pay[GA_IPT];
        uint64_t hb[GA_IPT];
        ga_load<false>(in, n, cb, gsh, key, pay, hb);
#pragma unroll
        for (int j = 0; j < GA_IPT; j++) {
            if (lane == 0) Lhb[w * GA_IPT + j] = hb[j];
            if (RANGE) Lkey[w * GA_CHUNK + 64 * j + lane] = key[j];
        }
    }
    __syncthreads();
    if (threadIdx.x < FR_WORDS) {
        const int x = threadIdx.x;
        int64_t p = -1, q = -1;
        for (int y = x - 1; y >= 0 && p < 0; y--)
            if (Lhb[y]) p = (int64_t)(tb + 64 * y + top_bit(Lhb[y]));
        for (int y = x + 1; y < (int)FR_WORDS && q < 0; y++)
            if (Lhb[y]) q = (int64_t)(tb + 64 * y + low_bit(Lhb[y]));
        Lprev[x] = p >= 0 ? p : g.hprev[blockIdx.x];
        Lnext[x] = q >= 0 ? q : (int64_t)g.hnext[blockIdx.x];
    }
    __syncthreads();
    const uint64_t le = lanemask_le();
#pragma unroll 1
    for (int j = 0; j < GA_IPT; j++) {
        const uint32_t word = w * GA_IPT + j;
        const uint64_t gi = cb + 64 * j + lane;
        if (gi >= n) continue;
        const int64_t i = (int64_t)gi;
        const uint64_t hm = Lhb[word] & le, am = Lhb[word] & ~le;
        // element 0 is a head: a block without one at or before the lane has
        // one in front of it
        const int64_t h = hm ? (int64_t)(tb + 64 * word + top_bit(hm)) : Lprev[word];
        const int64_t e = (am ? (int64_t)(tb + 64 * word + low_bit(am)) : Lnext[word]) - 1;
        int64_t a, b;
        bool empty = lo > hi;
        if (!RANGE) {
            int over;
            a = vmax(h, sat_add(i, lo, over));
            b = vmin(e, sat_add(i, hi, over));
        } else {
            const uint64_t te = min(tb + GA_TILE, n);
            int oa, ob;
            const int64_t k = Lkey[gi - tb];
            const int64_t ka = sat_add(k, lo, oa), kb = sat_add(k, hi, ob);
            // the first key >= ka: at or before the row when lo <= 0, behind it otherwise
            uint64_t lb, ub;
            if (ka == INT64_MIN) lb = (uint64_t)h;
            else if (lo <= 0) lb = frame_end_back<false>(in, Lkey, tb, (uint64_t)h, gi, ka);
            else lb = frame_end_fwd<false>(in, Lkey, tb, te, gi + 1, (uint64_t)e + 1, ka);
            // the first key > kb: behind the row when hi >= 0, at or before it otherwise
            if (kb == INT64_MAX) ub = (uint64_t)e + 1;
            else if (hi >= 0) ub = frame_end_fwd<true>(in, Lkey, tb, te, gi + 1, (uint64_t)e + 1, kb);
            else ub = frame_end_back<true>(in, Lkey, tb, (uint64_t)h, gi, kb);
            a = (int64_t)lb;
            b = (int64_t)ub - 1;
            empty = empty || oa > 0 || ob < 0;  // the band outside int64
        }
        empty = empty || a > b;
        int64_t sum = 0;
        MatVal mn = 0, mx = 0, first = 0, last = 0;
        if (!empty) {
            const uint64_t ua = (uint64_t)a, ub = (uint64_t)b;
            if (cols.first || (AGG && cols.sum)) first = mat_payload(in + ua);
            if (cols.last) last = mat_payload(in + ub);
            if (AGG && cols.sum) {
                const uint64_t pa = (uint64_t)g.texcl[ua / GA_TILE] + (uint64_t)g.pre[ua];
                const uint64_t pb = (uint64_t)g.texcl[ub / GA_TILE] + (uint64_t)g.pre[ub];
                sum = (int64_t)(pb - pa + (uint64_t)(int64_t)first);
            }
            if (AGG == 2) {
                const bool wmn = cols.mn != nullptr, wmx = cols.mx != nullptr;
                const uint64_t ba = ua / FR_BLOCK, bb = ub / FR_BLOCK;
                mn = kValMax;
                mx = kValMin;
                if (ba == bb) {
                    for (uint64_t p = ua; p <= ub; p++) {
                        const MatVal v = mat_payload(in + p);
                        mn = vmin(mn, v);
                        mx = vmax(mx, v);
                    }
                } else {
                    if (wmn) mn = vmin(g.smn[ua], g.pmn[ub]);
                    if (wmx) mx = vmax(g.smx[ua], g.pmx[ub]);
                    const uint64_t ta = ua / GA_TILE, tc = ub / GA_TILE;
                    if (ta == tc) {  // the blocks between them
                        for (uint64_t q = ba + 1; q < bb; q++) {
                            if (wmn) mn = vmin(mn, g.bmn[q]);
                            if (wmx) mx = vmax(mx, g.bmx[q]);
                        }
                    } else {
                        // the blocks behind a's in its tile, those in front of b's in its tile
                        if (ba + 1 < (ta + 1) * FR_WORDS) {
                            if (wmn) mn = vmin(mn, g.bsmn[ba + 1]);
                            if (wmx) mx = vmax(mx, g.bsmx[ba + 1]);
                        }
                        if (bb > tc * FR_WORDS) {
                            if (wmn) mn = vmin(mn, g.bpmn[bb - 1]);
                            if (wmx) mx = vmax(mx, g.bpmx[bb - 1]);
                        }
                        const uint64_t c = tc - ta - 1;  // whole tiles between
                        if (c) {
                            const uint32_t lv = top_bit(c);
                            const uint64_t x0 = (uint64_t)lv * g.ntiles + ta + 1;
                            const uint64_t x1 = (uint64_t)lv * g.ntiles + tc - (1ull << lv);
                            if (wmn) mn = vmin(mn, vmin(g.spmn[x0], g.spmn[x1]));
                            if (wmx) mx = vmax(mx, vmax(g.spmx[x0], g.spmx[x1]));
                        }
                    }
                }
            }
        }
        if (cols.start) st_col(cols.start + gi, empty ? (int64_t)-1 : a);
        if (cols.count) st_col(cols.count + gi, empty ? (int64_t)0 : b - a + 1);
        if (AGG && cols.sum) st_col(cols.sum + gi, sum);
        if (AGG == 2 && cols.mn) st_col(cols.mn + gi, mn);
        if (AGG == 2 && cols.mx) st_col(cols.mx + gi, mx);
        if (cols.first) st_col(cols.first + gi, first);
        if (cols.last) st_col(cols.last + gi, last);
    }
}

// the tables of a call in one scratch buffer, each 16-byte aligned
static FrameTab frame_tab(Workspace* ws, uint64_t n, const FrameCols& cols) {
    FrameTab g = {};
    g.ntiles = (n + GA_TILE - 1) / GA_TILE;
    const size_t nb = (size_t)((g.ntiles + GC_BLOCK - 1) / GC_BLOCK);  // scan workgroups
    g.levels = 1;
    while ((2ull << (g.levels - 1)) <= g.ntiles) g.levels++;
    const uint64_t nblocks = (n + FR_BLOCK - 1) / FR_BLOCK;
    const bool sum = cols.sum != nullptr;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += (bytes + 15) & ~(size_t)15;
        return at;
    };
    const size_t tile8 = g.ntiles * 8;
    const size_t o_tsum = take(sum ? tile8 : 0), o_texcl = take(sum ? tile8 : 0);
    const size_t o_tlast = take(tile8), o_hprev = take(tile8);
    const size_t o_tfirst = take(tile8), o_hnext = take(tile8);
    const size_t o_part = take(nb * sizeof(FCarry)), o_pexcl = take(nb * sizeof(FCarry));
    const size_t o_pre = take(sum ? n * 8 : 0);
    const size_t el = n * sizeof(MatVal), bl = nblocks * sizeof(MatVal);
    const size_t sp = (size_t)g.levels * g.ntiles * sizeof(MatVal);
    const size_t o_pmn = take(cols.mn ? el : 0), o_smn = take(cols.mn ? el : 0);
    const size_t o_pmx = take(cols.mx ? el : 0), o_smx = take(cols.mx ? el : 0);
    const size_t o_bmn = take(cols.mn ? 3 * bl : 0), o_bmx = take(cols.mx ? 3 * bl : 0);
    const size_t o_spmn = take(cols.mn ? sp : 0), o_spmx = take(cols.mx ? sp : 0);
    char* base = (char*)ws->scratch("frame_tab", off);
    if (sum) {
        g.tsum = (int64_t*)(base + o_tsum);
        g.texcl = (int64_t*)(base + o_texcl);
        g.pre = (int64_t*)(base + o_pre);
    }
    g.tlast = (int64_t*)(base + o_tlast);
    g.hprev = (int64_t*)(base + o_hprev);
    g.tfirst = (uint64_t*)(base + o_tfirst);
    g.hnext = (uint64_t*)(base + o_hnext);
    g.part = (FCarry*)(base + o_part);
    g.pexcl = (FCarry*)(base + o_pexcl);
    if (cols.mn) {
        g.pmn = (MatVal*)(base + o_pmn);
        g.smn = (MatVal*)(base + o_smn);
        g.bmn = (MatVal*)(base + o_bmn);
        g.bpmn = g.bmn + nblocks;
        g.bsmn = g.bpmn + nblocks;
        g.spmn = (MatVal*)(base + o_spmn);
    }
    if (cols.mx) {
        g.pmx = (MatVal*)(base + o_pmx);
        g.smx = (MatVal*)(base + o_smx);
        g.bmx = (MatVal*)(base + o_bmx);
        g.bpmx = g.bmx + nblocks;
        g.bsmx = g.bpmx + nblocks;
        g.spmx = (MatVal*)(base + o_spmx);
    }
    return g;
}

template <int AGG>
static void frame_passes(Workspace* ws, const Tup* in, uint64_t n, uint32_t gsh, bool range,
                         int64_t lo, int64_t hi, const FrameCols& cols, hipStream_t st) {
    const FrameTab g = frame_tab(ws, n, cols);
    const dim3 grid((uint32_t)g.ntiles), block(GA_THREADS);
    if constexpr (AGG != 0) {
        TraceScope ts(ws, "k_frame_build", st);
        hipLaunchKernelGGL(k_frame_build<AGG>, grid, block, 0, st, in, n, gsh, g);
        SMJ_CHECK(hipGetLastError());
    }
    {
        TraceScope ts(ws, "k_frame_scan", st);
        if (!AGG) {
            hipLaunchKernelGGL(k_frame_scan_heads, grid, block, 0, st, in, n, gsh, g);
            SMJ_CHECK(hipGetLastError());
        }
        carry_scan<FCarryOps>(ws, nullptr, FTiles{g.tsum, g.tlast, g.tfirst, g.ntiles}, g.ntiles,
                              CarryTable<FCarry>{g.part}, CarryTable<FCarry>{g.pexcl},
                              FFronts{g.texcl, g.hprev, g.hnext, g.ntiles, n}, st);
        if (AGG == 2) {
            for (uint32_t k = 1; k < g.levels; k++) {
                hipLaunchKernelGGL(k_frame_scan_sparse, dim3((uint32_t)((g.ntiles + 255) / 256)),
                                   dim3(256), 0, st, g, k);
                SMJ_CHECK(hipGetLastError());
            }
        }
    }
    TraceScope ts(ws, "k_frame_write", st);
    with_flag(range, [&](auto R) {
        hipLaunchKernelGGL((k_frame_write<AGG, decltype(R)::value>), grid, block, 0, st, in, n,
                           gsh, lo, hi, g, cols);
    });
    SMJ_CHECK(hipGetLastError());
}

void window_frame(Workspace* ws, const Tup* in, uint64_t n, uint32_t group_shift, bool range,
                  int64_t lo, int64_t hi, int64_t* start_out, int64_t* count_out,
                  int64_t* sum_out, void* min_out, void* max_out, void* first_out,
                  void* last_out, hipStream_t st) {
    const FrameCols cols{start_out, count_out, sum_out, (MatVal*)min_out, (MatVal*)max_out,
                         (MatVal*)first_out, (MatVal*)last_out};
    const int agg = (cols.mn || cols.mx) ? 2 : cols.sum ? 1 : 0;
    if (n == 0 || !(agg || cols.start || cols.count || cols.first || cols.last)) return;
    with_agg(agg, [&](auto A) {
        frame_passes<decltype(A)::value>(ws, in, n, group_shift, range, lo, hi, cols, st);
    });
}

}  // namespace smj
