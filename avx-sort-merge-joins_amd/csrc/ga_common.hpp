// ga_common.hpp -- what the kernels over the runs of one sorted relation
// share (groupagg.hip, window.hip): the tile geometry, the aggregate of some
// payloads and a tile's open tail, the lane moves, the chunk load with its
// head ballots, the segmented scan over the lanes of a wave and the block scan
// of the carry step.
#pragma once
#include "smj_common.hpp"
#include "mat_common.hpp"

namespace smj {

constexpr int GA_THREADS = MT_THREADS;
constexpr int GA_WAVES = GA_THREADS / 64;
constexpr int GA_IPT = 4;                             // rounds of 64 elements a wave
constexpr uint32_t GA_CHUNK = 64 * GA_IPT;            // consecutive elements of a wave
constexpr uint32_t GA_TILE = GA_WAVES * GA_CHUNK;     // elements of a workgroup
constexpr uint32_t GC_BLOCK = 1024;                   // tiles of a carry workgroup
constexpr uint64_t kNoHead = ~0ull;

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

// inclusive scan of one GCarry per thread over the workgroup (GC_BLOCK
// threads); *total = the whole workgroup's
__device__ __forceinline__ GCarry gc_block_scan(GCarry v, GCarry* wl, GCarry* total) {
    const int lane = lane_id(), wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        GCarry y;
        y.sum = sh_up(v.sum, o);
        y.mn = sh_up(v.mn, o);
        y.mx = sh_up(v.mx, o);
        y.start = (uint64_t)sh_up((int64_t)v.start, o);
        if (lane >= o) v = gc_comb(y, v);
    }
    if (lane == 63) wl[wid] = v;
    __syncthreads();
    GCarry p = gc_none(), all = gc_none();
#pragma unroll 1  // unrolled, the 16 entries are all loaded first (128 VGPRs and spills)
    for (int x = 0; x < (int)(GC_BLOCK / 64); x++) {
        if (x == wid) p = all;
        all = gc_comb(all, wl[x]);
    }
    *total = all;
    __syncthreads();  // wl is free again
    return gc_comb(p, v);
}

}  // namespace smj
