// mat_common.hpp -- what the join-output kernels over sorted R and S share
// (materialize.hip, bandjoin.hip, asofjoin.hip, outerjoin.hip): the tile
// geometry, the ABI's column type and its store, the key searches, the 64-bit
// block scan and tile sum, the staging of a tile's keys and R window in LDS,
// the walk over a tile's key runs with the per-tile bounds it starts from, and
// the work-item prologue and the per-output searches of the write passes.
#pragma once
#include <type_traits>
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

// one element of an output column
template <class T>
__device__ __forceinline__ void st_col(T* p, T v) {
#if SMJ_NT_STORES
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// k + d clamped to int64; over = +1 / -1 when the sum lay above / below it
// (the band join's and the window frames' key + lo, key + hi)
__device__ __forceinline__ int64_t sat_add(int64_t k, int64_t d, int& over) {
    int64_t r;
    over = 0;
    if (__builtin_add_overflow(k, d, &r)) {
        over = d > 0 ? 1 : -1;
        r = d > 0 ? INT64_MAX : INT64_MIN;
    }
    return r;
}

// key x lies in front of the first key >= k (UPPER: > k)
template <bool UPPER>
__device__ __forceinline__ bool key_before(int64_t x, int64_t k) {
    return UPPER ? x <= k : x < k;
}

// first index of [lo, hi) whose key is >= k (UPPER: > k), hi: none; K(i) = key
// i.  I is the index type: positions in a relation, or 32-bit offsets into
// staged keys (named by the caller, not deduced: common_type_t keeps it out)
template <bool UPPER, class I = uint64_t, class K>
__device__ __forceinline__ I key_search(K key, std::common_type_t<I> lo,
                                        std::common_type_t<I> hi, int64_t k) {
    while (lo < hi) {
        const I m = (lo + hi) >> 1;
        if (key_before<UPPER>(key(m), k)) lo = m + 1; else hi = m;
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
        if (!key_before<UPPER>(key(e), k)) return key_search<UPPER>(key, lo, e, k);
        lo = e + 1;
        step <<= 1;
    }
}

// the same answer, galloping backward from hi
template <bool UPPER, class I = uint64_t, class K>
__device__ __forceinline__ I key_gallop_back(K key, std::common_type_t<I> lo,
                                             std::common_type_t<I> hi, int64_t k) {
    I step = 1;
    while (hi - lo >= step && !key_before<UPPER>(key(hi - step), k)) {
        hi -= step;
        step <<= 1;
    }
    return key_search<UPPER, I>(key, hi - lo >= step ? hi - step + 1 : lo, hi, k);
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

// the sum of one uint64 per wave (the same in all its lanes) over the
// workgroup (MT_THREADS threads) into tile_out[blockIdx.x]; one barrier
__device__ __forceinline__ void tile_sum_store(uint64_t s, uint64_t* wsum,
                                               uint64_t* __restrict__ tile_out) {
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int w = 0; w < MT_THREADS / 64; w++) t += wsum[w];
        tile_out[blockIdx.x] = t;
    }
}

// the same of one uint64 per thread
__device__ __forceinline__ void tile_reduce_store(uint64_t s, uint64_t* wsum,
                                                  uint64_t* __restrict__ tile_out) {
    tile_sum_store(wave_sum(s), wsum, tile_out);
}

// ---- staging: the keys of S[tb, tb + len) and of the tile's R window
// R[Rlo, Rlo + W) in LDS.  Neither has a barrier: the caller places it.

__device__ __forceinline__ void stage_s_keys(const Tup* __restrict__ S, uint64_t tb,
                                             uint32_t len, int64_t* key) {
    for (uint32_t i = threadIdx.x; i < len; i += MT_THREADS) key[i] = tup_key(S[tb + i]);
}

// stages the window when it fits in MT_RWIN keys and says whether it did
// (uniform over the workgroup)
__device__ __forceinline__ bool stage_r_window(const Tup* __restrict__ R, uint64_t Rlo,
                                               uint64_t W, int64_t* rkey) {
    const bool staged = W <= MT_RWIN;
    if (staged)
        for (uint32_t i = threadIdx.x; i < W; i += MT_THREADS) rkey[i] = tup_key(R[Rlo + i]);
    return staged;
}

struct LdsKey {
    const int64_t* a;
    __device__ __forceinline__ int64_t operator()(uint64_t i) const { return a[i]; }
};

// f(K) with K(i) = key i of the window: from LDS when staged, else from R
template <class F>
__device__ __forceinline__ void with_window(bool staged, const int64_t* rkey,
                                            const Tup* __restrict__ R, uint64_t Rlo, F f) {
    if (staged) f(LdsKey{rkey});
    else f(TupKey{R + Rlo});
}

// ---- key runs: per tile the R window [0], [1] of its key range and the S
// extent of its first and last key runs [2], [3] (one thread per tile)

struct TileBounds {
    uint64_t tb, te;    // the tile's S range
    int64_t kf;         // its first key
    bool cont;          // the first run began in an earlier tile
    uint64_t rlo, rhi, s0, se;
    __device__ __forceinline__ void put(uint64_t* __restrict__ b) const {
        b[0] = rlo;
        b[1] = rhi;
        b[2] = s0;
        b[3] = se;
    }
};

__device__ __forceinline__ TileBounds tile_bounds(const Tup* __restrict__ R, uint64_t nR,
                                                  const Tup* __restrict__ S, uint64_t nS,
                                                  uint64_t t) {
    TileBounds x;
    x.tb = t * MT_TILE;
    x.te = min(x.tb + MT_TILE, nS);
    const TupKey rk{R}, sk{S};
    x.kf = sk(x.tb);
    const int64_t kl = sk(x.te - 1);
    x.rlo = key_search<false>(rk, 0, nR, x.kf);
    x.rhi = key_search<true>(rk, x.rlo, nR, kl);
    x.cont = x.tb > 0 && sk(x.tb - 1) == x.kf;
    x.s0 = x.cont ? key_search<false>(sk, 0, x.tb, x.kf) : x.tb;
    x.se = (x.te < nS && sk(x.te) == kl) ? key_search<true>(sk, x.te, nS, kl) : x.te;
    return x;
}

// The key runs of the thread's elements [i0, i1) of a tile of len keys L.key,
// and their R runs in the window of W keys at R position Rlo (K(i) = key i of
// it), each galloping on from the previous one.  What a mode keeps per element
// is its LDS struct's L.put_run(u, Rlo, rlo, rhi, s0, e): the R run
// [rlo, rhi) inside the window, and the tile indices of the element's run
// start (0: it may lie in an earlier tile, bounds word [2]) and run end (len:
// word [3]).
template <class K, class LDS>
__device__ __forceinline__ void run_walk(K rkey, uint64_t Rlo, uint64_t W, uint32_t i0,
                                         uint32_t i1, uint32_t len, LDS& L) {
    // run start of the thread's first element, run end of its last (LDS)
    uint32_t a = 0, b = i0;
    {
        const int64_t k = L.key[i0];
        while (a < b) {
            const uint32_t m = (a + b) >> 1;
            if (L.key[m] < k) a = m + 1; else b = m;
        }
    }
    uint32_t c = i1, d = len;
    {
        const int64_t k = L.key[i1 - 1];
        while (c < d) {
            const uint32_t m = (c + d) >> 1;
            if (L.key[m] <= k) c = m + 1; else d = m;
        }
    }
    uint32_t s0 = a;
    uint64_t rlo, rhi = 0;
    uint32_t i = i0;
    while (i < i1) {
        const int64_t k = L.key[i];
        uint32_t j = i + 1;
        while (j < i1 && L.key[j] == k) j++;
        if (i != i0) s0 = i;
        rlo = key_gallop<false>(rkey, rhi, W, k);
        rhi = key_gallop<true>(rkey, rlo, W, k);
        const uint32_t e = j < i1 ? j : c;
        for (uint32_t u = i; u < j; u++) L.put_run(u, Rlo, rlo, rhi, s0, e);
        i = j;
    }
}

// The tile pass of the run-based kernels: the tile's WORDS bounds words into
// L.ends, its S keys and (when it fits) its R window's keys `rkey` staged, then
// the walk.  Every thread of the workgroup calls it; two barriers, none after
// the walk.
template <uint32_t WORDS, class LDS>
__device__ __forceinline__ void run_tile(const Tup* __restrict__ R, const Tup* __restrict__ S,
                                         const uint64_t* __restrict__ bounds, uint64_t t,
                                         uint64_t tb, uint32_t len, LDS& L, int64_t* rkey) {
    const uint32_t tid = threadIdx.x;
    if (tid < WORDS) L.ends[tid] = bounds[WORDS * t + tid];
    stage_s_keys(S, tb, len, L.key);
    __syncthreads();
    const uint64_t Rlo = L.ends[0], W = L.ends[1] - Rlo;
    const bool staged = stage_r_window(R, Rlo, W, rkey);
    __syncthreads();
    const uint32_t i0 = tid * MT_IPT;
    if (i0 >= len) return;
    const uint32_t i1 = min(i0 + (uint32_t)MT_IPT, len);
    with_window(staged, rkey, R, Rlo, [&](auto rk) { run_walk(rk, Rlo, W, i0, i1, len, L); });
}

// the S extent [s0, se) of element j's key run, from the uint16 entries
__device__ __forceinline__ void run_extent(const uint16_t* ls0, const uint16_t* lse, uint32_t j,
                                           uint64_t tb, uint32_t len, int64_t first_s0,
                                           int64_t last_se, int64_t& s0, int64_t& se) {
    const uint32_t a = ls0[j], c = lse[j];
    s0 = a == 0 ? first_s0 : (int64_t)(tb + a);
    se = c == len ? last_se : (int64_t)(tb + c);
}

// pair `off` of a run of sc S tuples, R-major: d = the R tuple off / sc of the
// run; returns the S tuple off % sc
__device__ __forceinline__ uint64_t run_pair(uint64_t off, uint64_t sc, uint64_t& d) {
    d = off;
    if (sc != 1) d = ((off | sc) >> 32) ? off / sc : (uint32_t)off / (uint32_t)sc;
    return off - d * sc;
}

// ---- the write passes: one workgroup per work item of kMatPiece outputs

struct MatPiece {
    uint64_t t;       // the tile that owns the item
    uint64_t q0, q1;  // the item's outputs, counted inside the tile
    uint64_t ob;      // the tile's first output
    uint64_t tb;      // the tile's first S element
    uint32_t len;     // its S elements
    bool live;        // some output lies below out_cap (uniform over the workgroup)
};

// work item blockIdx.x; every thread of the workgroup calls it (one barrier)
__device__ __forceinline__ MatPiece mat_piece(const uint64_t* __restrict__ ibase,
                                              const uint64_t* __restrict__ cnt,
                                              const uint64_t* __restrict__ base,
                                              uint64_t ntiles, uint64_t nS, uint64_t out_cap,
                                              uint64_t* sh_t) {
    const uint64_t w = blockIdx.x;
    if (threadIdx.x == 0) {
        // the last tile whose first item is <= w owns item w
        uint64_t lo = 0, hi = ntiles;
        while (lo < hi) {
            const uint64_t m = (lo + hi) >> 1;
            if (ibase[m] <= w) lo = m + 1; else hi = m;
        }
        *sh_t = lo - 1;
    }
    __syncthreads();
    MatPiece p;
    p.t = *sh_t;
    p.q0 = (w - ibase[p.t]) * kMatPiece;
    p.q1 = min(p.q0 + kMatPiece, cnt[p.t]);
    p.ob = base[p.t];
    p.live = p.ob + p.q0 < out_cap;
    p.tb = p.t * MT_TILE;
    p.len = (uint32_t)min((uint64_t)MT_TILE, nS - p.tb);
    return p;
}

// the first of the inclusive prefixes pre[0..n] that lies above q (pre[n] > q)
__device__ __forceinline__ uint32_t prefix_pick(const uint64_t* pre, uint32_t n, uint64_t q) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if (pre[m] <= q) lo = m + 1; else hi = m;
    }
    return lo;
}

}  // namespace smj
