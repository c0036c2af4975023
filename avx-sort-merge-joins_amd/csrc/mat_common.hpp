// mat_common.hpp -- what the join-output kernels over sorted R and S share
// (materialize.hip, bandjoin.hip): the tile geometry, the ABI's column type,
// the key searches and the 64-bit block scan.
#pragma once
#include "smj_common.hpp"

namespace smj {

constexpr int MT_THREADS = 256;
// small tiles keep the LDS per workgroup at 18 KB (8 workgroups per CU), so
// the staging loads of some workgroups overlap the searches of others
// (16 B, 128M x 128M, before the bitmap path: 2048-element tiles 6.6 ms,
// 1024: 4.6 ms, 512: 4.2 ms; with it: 1024: 2.9 ms, 512: 2.4 ms, 256: 3.7 ms
// -- more, smaller tiles lose to the per-tile searches and launch width)
constexpr int MT_IPT = 2;
constexpr uint32_t MT_TILE = MT_THREADS * MT_IPT;  // S elements per tile
constexpr uint32_t MT_RWIN = 2 * MT_TILE;          // R keys staged in LDS
constexpr uint64_t kMatPiece = 8192;                // outputs per work item

#ifdef KEY_8B
typedef int64_t MatVal;  // value_t and intkey_t of the C ABI
#else
typedef int32_t MatVal;
#endif

__device__ __forceinline__ MatVal mat_payload(const Tup* p) {
#ifdef KEY_8B
    return p->payload;
#else
    return (MatVal)(uint32_t)*p;
#endif
}

__device__ __forceinline__ void st_val(MatVal* p, MatVal v) {
#if SMJ_NT_STORES
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// first index of [lo, hi) whose key is >= k (UPPER: > k); K(i) = key i
template <bool UPPER, class K>
__device__ __forceinline__ uint64_t key_search(K key, uint64_t lo, uint64_t hi,
                                               int64_t k) {
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        const int64_t x = key(m);
        if (UPPER ? x <= k : x < k) lo = m + 1; else hi = m;
    }
    return lo;
}

// the same answer, galloping forward from lo (consecutive keys of a tile sit
// close together in R)
template <bool UPPER, class K>
__device__ __forceinline__ uint64_t key_gallop(K key, uint64_t lo, uint64_t hi,
                                               int64_t k) {
    uint64_t step = 1;
    while (true) {
        const uint64_t e = lo + step - 1;
        if (e >= hi) return key_search<UPPER>(key, lo, hi, k);
        const int64_t x = key(e);
        if (!(UPPER ? x <= k : x < k)) return key_search<UPPER>(key, lo, e, k);
        lo = e + 1;
        step <<= 1;
    }
}

struct TupKey {
    const Tup* a;
    __device__ __forceinline__ int64_t operator()(uint64_t i) const { return tup_key(a[i]); }
};

// block-wide exclusive scan of one uint64 per thread
__device__ __forceinline__ uint64_t block_scan64(uint64_t v, uint64_t* wsum,
                                                 uint64_t* total) {
    const int lane = lane_id(), wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int w = 0; w < nw; w++) {
            const uint64_t t = wsum[w];
            wsum[w] = run;
            run += t;
        }
        wsum[nw] = run;
    }
    __syncthreads();
    const uint64_t res = wsum[wid] + x - v;
    if (total) *total = wsum[nw];
    __syncthreads();
    return res;
}

}  // namespace smj
