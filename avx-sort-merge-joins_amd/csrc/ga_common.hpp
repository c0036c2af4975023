// ga_common.hpp -- what the operators over the runs of one sorted relation
// share (groupagg.hip, window.hip, frame.hip): the tile geometry, the aggregate
// of some payloads and a tile's open tail, the lane moves, the chunk load with
// its head ballots, the segmented scan over the lanes of a wave, a wave's open
// tail (the count passes), the walk over a wave's chunk and what
// comes in to it (the write passes), the carry step over the tiles (one block
// scan and three kernels over any carried struct), the tile table with the
// carry step's tables, and the dispatch on the aggregate level.  A new operator
// of the family brings its column struct, its carried struct with none(),
// comb() and the lane move (a CarryOps), and what it does per element.
#pragma once
#include <type_traits>
#include "smj_common.hpp"
#include "smj_internal.hpp"
#include "mat_common.hpp"

namespace smj {

constexpr int GA_THREADS = MT_THREADS;
constexpr int GA_WAVES = GA_THREADS / 64;
constexpr int GA_IPT = 4;                             // rounds of 64 elements a wave
constexpr uint32_t GA_CHUNK = 64 * GA_IPT;            // consecutive elements of a wave
constexpr uint32_t GA_TILE = GA_WAVES * GA_CHUNK;     // elements of a workgroup
constexpr uint32_t GC_BLOCK = 1024;                   // tiles of a carry workgroup
constexpr uint64_t kNoHead = ~0ull;
constexpr uint32_t kNoOff = ~0u;  // a head as an offset in the chunk: in front of it

// sum, minimum and maximum of some payloads, in registers
struct GAgg {
    int64_t sum;
    MatVal mn, mx;
};

#ifdef KEY_8B
constexpr MatVal kValMax = INT64_MAX, kValMin = INT64_MIN;
#else
constexpr MatVal kValMax = INT32_MAX, kValMin = INT32_MIN;
#endif

__device__ __forceinline__ GAgg ga_none() { return GAgg{0, kValMax, kValMin}; }
__device__ __forceinline__ GAgg ga_one(MatVal p) { return GAgg{(int64_t)p, p, p}; }

template <class T>
__device__ __forceinline__ T vmin(T a, T b) { return b < a ? b : a; }
template <class T>
__device__ __forceinline__ T vmax(T a, T b) { return b > a ? b : a; }

__device__ __forceinline__ GAgg ga_comb(const GAgg& a, const GAgg& b) {
    return GAgg{(int64_t)((uint64_t)a.sum + (uint64_t)b.sum), vmin(a.mn, b.mn), vmax(a.mx, b.mx)};
}

// a tile's (a range of tiles') open tail in the tables: the aggregate behind
// its last head, at `start`, or of all of it when it has none (kNoHead)
struct GCarry {
    int64_t sum, mn, mx;
    uint64_t start;
};

// (the ends of the payload type, so that the tables' values always fit it)
__device__ __forceinline__ GCarry gc_none() {
    return GCarry{0, (int64_t)kValMax, (int64_t)kValMin, kNoHead};
}

// a then b: a head in b closes what a left open.  Field by field: a select
// between two structs can go through scratch memory
__device__ __forceinline__ GCarry gc_comb(const GCarry& a, const GCarry& b) {
    const bool cut = b.start != kNoHead;
    GCarry r;
    r.sum = cut ? b.sum : (int64_t)((uint64_t)a.sum + (uint64_t)b.sum);
    r.mn = cut ? b.mn : vmin(a.mn, b.mn);
    r.mx = cut ? b.mx : vmax(a.mx, b.mx);
    r.start = cut ? b.start : a.start;
    return r;
}

// Lane moves of the scans as DPP modifiers of VALU moves (row_shr:n inside a
// row of 16 lanes, row_bcast:15 / row_bcast:31 across rows, wave_shr:1), not
// ds_bpermute: the write pass is bound by them.  A lane without a source keeps
// its own value.
constexpr int kDppRowShr = 0x110, kDppWaveShr1 = 0x138, kDppBcast15 = 0x142,
              kDppBcast31 = 0x143;

template <int CTRL, int ROWS>
__device__ __forceinline__ int32_t dpp(int32_t v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ int64_t dpp(int64_t v) {
    const uint32_t lo = (uint32_t)dpp<CTRL, ROWS>((int32_t)(uint32_t)v);
    const uint32_t hi = (uint32_t)dpp<CTRL, ROWS>((int32_t)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// the value of lane 63, in every lane
__device__ __forceinline__ int32_t last_lane(int32_t v) {
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int64_t last_lane(int64_t v) {
    const uint32_t lo = (uint32_t)last_lane((int32_t)(uint32_t)v);
    const uint32_t hi = (uint32_t)last_lane((int32_t)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int64_t sh_up(int64_t v, int o) {
    return (int64_t)__shfl_up((unsigned long long)v, o, 64);
}
__device__ __forceinline__ int32_t sh_up(int32_t v, int o) { return __shfl_up(v, o, 64); }
__device__ __forceinline__ int64_t sh_xor(int64_t v, int o) {
    return (int64_t)__shfl_xor((unsigned long long)v, o, 64);
}
__device__ __forceinline__ int32_t sh_xor(int32_t v, int o) { return __shfl_xor(v, o, 64); }

__device__ __forceinline__ int64_t ga_key(const Tup* p) {
#ifdef KEY_8B
    return p->key;
#else
    return (int64_t)reinterpret_cast<const int32_t*>(p)[1];
#endif
}

// position of the highest set bit of a non-zero mask
__device__ __forceinline__ uint32_t top_bit(uint64_t m) {
    return 63u - (uint32_t)__clzll((long long)m);
}

// the lanes at or below this one
__device__ __forceinline__ uint64_t lanemask_le() { return (2ull << lane_id()) - 1; }

// The wave's chunk [cb, cb + GA_CHUNK) of `in`: keys and (PAY) payloads of the
// elements inside the relation, and per round the ballot of the heads.
template <bool PAY>
__device__ __forceinline__ void ga_load(const Tup* __restrict__ in, uint64_t n, uint64_t cb,
                                        uint32_t gsh, int64_t (&key)[GA_IPT],
                                        MatVal (&pay)[GA_IPT], uint64_t (&hb)[GA_IPT]) {
    const int lane = lane_id();
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        const uint64_t gi = cb + 64 * j + lane;
        key[j] = 0;
        pay[j] = 0;
        if (gi < n) {
            if (PAY) {
                const Tup t = in[gi];
                key[j] = tup_key(t);
                pay[j] = mat_payload(&t);
            } else {
                key[j] = ga_key(in + gi);
            }
        }
    }
    // the group in front of the chunk (the same address in every lane)
    int64_t last = 0;
    if (cb > 0 && cb < n) last = ga_key(in + cb - 1) >> gsh;
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        const uint64_t gi = cb + 64 * j + lane;
        const int64_t g = key[j] >> gsh;
        int64_t pg = dpp<kDppWaveShr1, 0xf>(g);
        if (lane == 0) pg = last;
        hb[j] = __ballot(gi < n && (gi == 0 || g != pg));
        last = last_lane(g);
    }
}

template <int CTRL, int ROWS>
__device__ __forceinline__ GAgg ga_dpp(const GAgg& v) {
    return GAgg{dpp<CTRL, ROWS>(v.sum), dpp<CTRL, ROWS>(v.mn), dpp<CTRL, ROWS>(v.mx)};
}

// Inclusive segmented scan over the lanes of a wave: d = the lanes of this
// lane's segment in front of it.  Four steps inside the rows of 16 lanes;
// then rows 1 and 3 take the last lane of the row in front, and rows 2 and 3
// lane 31, each lane only as far as its segment reaches.  (What lane 15, 31
// or 47 holds by then covers its own segment, which is the taker's.)
__device__ __forceinline__ GAgg ga_seg_scan(GAgg v, int d) {
    const int lane = lane_id(), r = lane & 15;
    GAgg y;
    y = ga_dpp<kDppRowShr + 1, 0xf>(v);
    if (r >= 1 && d >= 1) v = ga_comb(y, v);
    y = ga_dpp<kDppRowShr + 2, 0xf>(v);
    if (r >= 2 && d >= 2) v = ga_comb(y, v);
    y = ga_dpp<kDppRowShr + 4, 0xf>(v);
    if (r >= 4 && d >= 4) v = ga_comb(y, v);
    y = ga_dpp<kDppRowShr + 8, 0xf>(v);
    if (r >= 8 && d >= 8) v = ga_comb(y, v);
    y = ga_dpp<kDppBcast15, 0xa>(v);
    if ((lane & 16) && d > r) v = ga_comb(y, v);
    y = ga_dpp<kDppBcast31, 0xc>(v);
    if (lane >= 32 && d >= lane - 31) v = ga_comb(y, v);
    return v;
}

// ---- a chunk's and a tile's open tail

struct GWave {  // what a wave leaves for the others of its tile
    GCarry tail;
    uint32_t heads;
};

// the tail of an aggregate behind the head at `start`; AGG 0: the position
// alone, 1: with the sum, 2: with minimum and maximum as well
template <int AGG>
__device__ __forceinline__ GCarry gc_tail(const GAgg& a, uint64_t start) {
    return GCarry{a.sum, AGG == 2 ? (int64_t)a.mn : 0, AGG == 2 ? (int64_t)a.mx : 0, start};
}

// The count passes' wave: the heads of its chunk and its open tail, the
// aggregate from its last head to its end (of all of it when it has no head),
// into *out.
template <int AGG>
__device__ __forceinline__ void ga_wave_tail(uint64_t n, uint64_t cb,
                                             const MatVal (&pay)[GA_IPT],
                                             const uint64_t (&hb)[GA_IPT], GWave* out) {
    const int lane = lane_id();
    uint32_t heads = 0;
    uint32_t lso = kNoOff;  // the chunk's last head
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        heads += (uint32_t)__popcll(hb[j]);
        if (hb[j]) lso = 64 * j + top_bit(hb[j]);
    }
    GAgg a = ga_none();
    if (AGG) {
        // the chunk's elements inside the relation
        const uint32_t len = cb < n ? (uint32_t)min(n - cb, (uint64_t)GA_CHUNK) : 0;
#pragma unroll
        for (int j = 0; j < GA_IPT; j++) {
            const uint32_t o = 64 * j + lane;
            // behind the last head, or everything
            const bool in_tail = o < len && (lso == kNoOff || o >= lso);
            if (in_tail) a = ga_comb(a, ga_one(pay[j]));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            a = ga_comb(a, GAgg{sh_xor(a.sum, o), sh_xor(a.mn, o), sh_xor(a.mx, o)});
    }
    if (lane == 0) {
        out->tail = gc_tail<AGG>(a, lso == kNoOff ? kNoHead : cb + lso);
        out->heads = heads;
    }
}

// The write passes' walk over the wave's chunk.  Per element: x = the aggregate
// from its head, or from the chunk's start, to it (AGG), so = its head as an
// offset in the chunk (kNoOff: in front of the chunk), hrank = the heads of the
// chunk at or before it.  Returns what the wave leaves (the same in every lane).
template <int AGG>
__device__ __forceinline__ GWave ga_walk(uint64_t n, uint64_t cb, const MatVal (&pay)[GA_IPT],
                                         const uint64_t (&hb)[GA_IPT], GAgg (&x)[GA_IPT],
                                         uint32_t (&so)[GA_IPT], uint32_t (&hrank)[GA_IPT]) {
    const int lane = lane_id();
    const uint64_t le = lanemask_le();
    GAgg run = ga_none();  // the open tail of the rounds so far
    uint32_t rso = kNoOff, heads = 0;
#pragma unroll
    for (int j = 0; j < GA_IPT; j++) {
        const uint64_t hm = hb[j] & le;  // the round's heads at or before this lane
        const uint32_t seg = hm ? top_bit(hm) : 0;
        if (AGG) {
            GAgg v = cb + 64 * j + lane < n ? ga_one(pay[j]) : ga_none();
            v = ga_seg_scan(v, lane - (int)seg);
            if (!hm) v = ga_comb(run, v);
            x[j] = v;
            run = GAgg{last_lane(v.sum), last_lane(v.mn), last_lane(v.mx)};
        }
        so[j] = hm ? 64 * j + seg : rso;
        hrank[j] = heads + (uint32_t)__popcll(hm);
        if (hb[j]) rso = 64 * j + top_bit(hb[j]);
        heads += (uint32_t)__popcll(hb[j]);
    }
    return GWave{gc_tail<AGG>(run, rso == kNoOff ? kNoHead : cb + rso), heads};
}

// what comes in to wave w: the tile's carry `inc` and first row `row`, with
// the tails and heads of the earlier waves of the tile
__device__ __forceinline__ void ga_incoming(const GWave* L, int w, GCarry& inc, uint64_t& row) {
#pragma unroll
    for (int v = 0; v < GA_WAVES - 1; v++) {
        if (v < w) {
            inc = gc_comb(inc, L[v].tail);
            row += L[v].heads;
        }
    }
}

// ---- the carry step: an inclusive scan over the tiles of what each leaves
// open, GC_BLOCK tiles a workgroup, in three kernels (no workgroup waits for
// another).  Ops names the carried struct T with none(), comb(a, b) (a then b)
// and up(v, o), v of the lane o below.  up() moves field by field: a select
// between two structs can go through scratch memory.  The tables are accessors
// with load(i) / store(i, v), so that an operator may keep the fields of T in
// tables of its own.

template <class T>
struct CarryShared {
    T a[GC_BLOCK / 64];
    __device__ __forceinline__ void put(int i, const T& v) { a[i] = v; }
    __device__ __forceinline__ T get(int i) const { return a[i]; }
};

struct GCarryOps {
    typedef GCarry T;
    typedef CarryShared<GCarry> Shared;
    static __device__ __forceinline__ T none() { return gc_none(); }
    static __device__ __forceinline__ T comb(const T& a, const T& b) { return gc_comb(a, b); }
    static __device__ __forceinline__ T up(const T& v, int o) {
        T y;
        y.sum = sh_up(v.sum, o);
        y.mn = sh_up(v.mn, o);
        y.mx = sh_up(v.mx, o);
        y.start = (uint64_t)sh_up((int64_t)v.start, o);
        return y;
    }
};

template <class T>
struct CarryTable {  // one array of T
    T* p;
    __device__ __forceinline__ T load(uint64_t i) const { return p[i]; }
    __device__ __forceinline__ void store(uint64_t i, const T& v) const { p[i] = v; }
};

// inclusive scan of one T per thread over the workgroup (GC_BLOCK threads);
// *total = the whole workgroup's
template <class Ops>
__device__ __forceinline__ typename Ops::T carry_block_scan(typename Ops::T v,
                                                            typename Ops::Shared& wl,
                                                            typename Ops::T* total) {
    typedef typename Ops::T T;
    const int lane = lane_id(), wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = Ops::up(v, o);
        if (lane >= o) v = Ops::comb(y, v);
    }
    if (lane == 63) wl.put(wid, v);
    __syncthreads();
    T p = Ops::none(), all = Ops::none();
#pragma unroll 1  // unrolled, the 16 entries are all loaded first (128 VGPRs and spills)
    for (int x = 0; x < (int)(GC_BLOCK / 64); x++) {
        if (x == wid) p = all;
        all = Ops::comb(all, wl.get(x));
    }
    *total = all;
    __syncthreads();  // wl is free again
    return Ops::comb(p, v);
}

// per GC_BLOCK items: their combination
template <class Ops, class In, class Part>
__global__ void __launch_bounds__(GC_BLOCK) k_carry_part(In in, uint64_t n, Part part) {
    typedef typename Ops::T T;
    __shared__ typename Ops::Shared wl;
    const uint64_t t = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    T all;
    carry_block_scan<Ops>(t < n ? in.load(t) : Ops::none(), wl, &all);
    if (threadIdx.x == 0) part.store(blockIdx.x, all);
}

// pexcl[b] = the parts in front of workgroup b combined (one workgroup)
template <class Ops, class Part>
__global__ void __launch_bounds__(GC_BLOCK) k_carry_pscan(Part part, uint32_t nb, Part pexcl) {
    typedef typename Ops::T T;
    __shared__ typename Ops::Shared wl;
    T run = Ops::none();
    if (threadIdx.x == 0) pexcl.store(0, run);
    for (uint32_t r0 = 0; r0 < nb; r0 += GC_BLOCK) {
        const uint32_t b = r0 + threadIdx.x;
        T all;
        const T inc = carry_block_scan<Ops>(b < nb ? part.load(b) : Ops::none(), wl, &all);
        if (b + 1 < nb) pexcl.store(b + 1, Ops::comb(run, inc));
        run = Ops::comb(run, all);
    }
}

// carry[t] = all items in front of item t combined
template <class Ops, class In, class Part, class Out>
__global__ void __launch_bounds__(GC_BLOCK)
k_carry_down(In in, uint64_t n, Part pexcl, Out carry) {
    typedef typename Ops::T T;
    __shared__ typename Ops::Shared wl;
    const uint64_t t = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    T all;
    const T inc = carry_block_scan<Ops>(t < n ? in.load(t) : Ops::none(), wl, &all);
    const T front = pexcl.load(blockIdx.x);
    if (t == 0) carry.store(0, front);
    if (t + 1 < n) carry.store(t + 1, Ops::comb(front, inc));
}

// the three launches, traced as `name` (null: inside the caller's scope)
template <class Ops, class In, class Part, class Out>
static void carry_scan(Workspace* ws, const char* name, In in, uint64_t n, Part part, Part pexcl,
                       Out carry, hipStream_t st) {
    TraceScope ts(name ? ws : nullptr, name, st);
    const uint32_t nb = (uint32_t)((n + GC_BLOCK - 1) / GC_BLOCK);
    hipLaunchKernelGGL((k_carry_part<Ops, In, Part>), dim3(nb), dim3(GC_BLOCK), 0, st, in, n,
                       part);
    SMJ_CHECK(hipGetLastError());
    hipLaunchKernelGGL((k_carry_pscan<Ops, Part>), dim3(1), dim3(GC_BLOCK), 0, st, part, nb,
                       pexcl);
    SMJ_CHECK(hipGetLastError());
    hipLaunchKernelGGL((k_carry_down<Ops, In, Part, Out>), dim3(nb), dim3(GC_BLOCK), 0, st, in, n,
                       pexcl, carry);
    SMJ_CHECK(hipGetLastError());
}

// ---- the tile table of the operators that carry tails

// the key level of an open tail (window.hip): its last key head (kNoHead:
// none) and the key-only heads behind its last group head (in all of it when
// it has none)
struct KCarry {
    uint64_t kstart, dense;
};

// materialize.hip's tile table with 0 bounds words (`bounds` is unused and
// equals `tot`) and, in tile_tab's extra bytes behind tot[0..1], the carry
// step's tables: tail, carry (a tile), part, pexcl (a carry workgroup), and
// with `keys` the same four of the key level behind them
struct TailTab : TileTab {
    GCarry *tail, *carry, *part, *pexcl;
    KCarry *ktail, *kcarry, *kpart, *kpexcl;  // null without `keys`
};

static TailTab tail_tab(Workspace* ws, const char* scratch_name, uint64_t n, bool keys) {
    TailTab g;
    const uint64_t ntiles = (n + GA_TILE - 1) / GA_TILE;
    const size_t nb = (size_t)((ntiles + GC_BLOCK - 1) / GC_BLOCK);
    const size_t pad = ((3 * ntiles) & 1) * 8;  // the carry tables 16-aligned
    const size_t items = 2 * ntiles + 2 * nb;
    static_cast<TileTab&>(g) = tile_tab(
        ws, scratch_name, ntiles, 0,
        pad + items * (sizeof(GCarry) + (keys ? sizeof(KCarry) : 0)));
    g.tail = (GCarry*)((char*)(g.tot + 2) + pad);
    g.carry = g.tail + ntiles;
    g.part = g.carry + ntiles;
    g.pexcl = g.part + nb;
    g.ktail = keys ? (KCarry*)(g.pexcl + nb) : nullptr;
    g.kcarry = keys ? g.ktail + ntiles : nullptr;
    g.kpart = keys ? g.kcarry + ntiles : nullptr;
    g.kpexcl = keys ? g.kpart + nb : nullptr;
    return g;
}

// the carry step over the tails alone, traced as `name` (groupagg.hip)
void tail_carry(Workspace* ws, const char* name, const TailTab& g, hipStream_t st);

// ---- dispatch: f(std::integral_constant) of the aggregate level 0..2, of a flag

template <class F>
static void with_agg(int agg, F f) {
    if (agg == 2) f(std::integral_constant<int, 2>{});
    else if (agg == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

template <class F>
static void with_flag(bool on, F f) {
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace smj

