// asofjoin.hip -- as-of join of two sorted relations (smj.h smj_dev_asof_join):
// for every S tuple ONE partner in sorted R, the last tuple at or before its
// key (backward), the first at or after it (forward) or the closer of the two
// (nearest), within a tolerance and inside the same key group.  The library's
// own; the reference has equality joins only.
//
// With lb the first position of sorted R whose key is >= s.key and ub the
// first whose key is > s.key (both non-decreasing along sorted S), the two
// candidates of an S tuple are
//   B = ub - 1, F = lb        equal keys are partners,
//   B = lb - 1, F = ub        strict;
// B exists when it is >= 0 and F when it is < nR.  Each is filtered on its own
// by the tolerance and the group; nearest takes the survivor at the smaller
// distance, B on equal distances.  Distances are uint64 differences of the
// int64 keys (B's key <= s.key <= F's key: nothing wraps).
//
// Every S tuple has exactly one output row, so there is no count pass, no
// scan and no host synchronisation:
//   k_asof_bounds one thread per S tile: the tile's R window, from one below
//                 the lower bound of its first key to one past the upper bound
//                 of its last, so the B of the first element and the F of the
//                 last lie inside it (clamped to R);
//   k_asof_tile   one workgroup per S tile: the tile's keys and (when it
//                 fits) the window's keys staged in LDS; per element the two
//                 bounds, each galloping on from the previous element's, the
//                 candidates, the filters and the choice; the partner's
//                 position replaces the element's key in LDS; after a barrier
//                 thread i of each round reads element i's partner tuple from
//                 R and writes row tb + i of every column (coalesced), and
//                 the tile's matched rows go to a table;
//   k_asof_total  the table summed into *matched_dev by materialize.hip's
//                 tile_total (only when the caller asks for the count).
#include "smj_common.hpp"
#include "smj_internal.hpp"
#include "mat_common.hpp"

namespace smj {

// the output columns (each may be null)
struct AsofCols {
    int64_t* idx;
    MatVal* pay;
    MatVal* key;
};

// how the two candidates are formed, filtered and chosen
struct AsofMode {
    uint32_t dir;     // kAsofBackward, kAsofForward, kAsofNearest
    uint32_t strict;  // equal keys are no partners
    uint32_t gsh;     // group shift, 0: no groups
    uint64_t tol;     // largest distance
};

// per tile: its R window [max(lb(first key) - 1, 0), min(ub(last key) + 1, nR))
__global__ void __launch_bounds__(256)
k_asof_bounds(const Tup* __restrict__ R, uint64_t nR, const Tup* __restrict__ S, uint64_t nS,
              uint64_t ntiles, uint64_t* __restrict__ bounds) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const uint64_t tb = t * MT_TILE;
    const uint64_t te = min(tb + MT_TILE, nS);
    const TupKey rk{R}, sk{S};
    const uint64_t lb = key_search<false>(rk, 0, nR, sk(tb));
    const uint64_t ub = key_search<true>(rk, lb, nR, sk(te - 1));  // last key >= first key
    bounds[2 * t + 0] = lb ? lb - 1 : 0;
    bounds[2 * t + 1] = ub < nR ? ub + 1 : nR;
}

struct AsofLDS {
    int64_t key[MT_TILE];   // the S keys, then each element's partner (position in R, -1: none)
    int64_t rkey[MT_RWIN];  // the R window's keys, when it fits
    uint32_t wsum[MT_THREADS / 64];
};

// does the candidate with key r count for the S key k at distance d
__device__ __forceinline__ bool asof_ok(const AsofMode& m, int64_t r, int64_t k, uint64_t d) {
    return d <= m.tol && (m.gsh == 0 || (r >> m.gsh) == (k >> m.gsh));
}

// partners of the thread's elements [i0, i0 + MT_IPT) of a tile of len in the
// window R[Rlo, Rlo + W) (K(i) = key i of it): skey[i] becomes the partner's
// position in R or -1; returns the number of matched elements
template <class K>
__device__ __forceinline__ uint32_t asof_partners(K rkey, uint64_t Rlo, uint64_t W, int64_t* skey,
                                                  uint32_t i0, uint32_t len, const AsofMode& m) {
    uint64_t lb = 0, ub = 0;
    uint32_t matched = 0;
#pragma unroll
    for (uint32_t p = 0; p < MT_IPT; p++) {
        if (i0 + p < len) {
            const int64_t k = skey[i0 + p];
            lb = key_gallop<false>(rkey, lb, W, k);
            ub = key_gallop<true>(rkey, max(ub, lb), W, k);
            const uint64_t b = m.strict ? lb : ub;  // B is at b - 1
            const uint64_t f = m.strict ? ub : lb;  // F is at f
            // the window reaches one past both ends of the tile's keys: b == 0
            // or f == W only where R itself ends (k_asof_bounds)
            bool okb = m.dir != kAsofForward && b > 0;
            bool okf = m.dir != kAsofBackward && f < W;
            uint64_t db = 0, df = 0;
            if (okb) {
                const int64_t r = rkey(b - 1);  // r <= k
                db = (uint64_t)k - (uint64_t)r;
                okb = asof_ok(m, r, k, db);
            }
            if (okf) {
                const int64_t r = rkey(f);  // r >= k
                df = (uint64_t)r - (uint64_t)k;
                okf = asof_ok(m, r, k, df);
            }
            int64_t q = -1;
            if (okb && (!okf || db <= df)) q = (int64_t)(Rlo + b - 1);
            else if (okf) q = (int64_t)(Rlo + f);
            skey[i0 + p] = q;  // no other thread reads this element before the barrier
            matched += q >= 0;
        }
    }
    return matched;
}

// tile_out null: the caller does not ask for the matched count
__global__ void __launch_bounds__(MT_THREADS)
k_asof_tile(const Tup* __restrict__ R, const Tup* __restrict__ S, uint64_t nS,
            const uint64_t* __restrict__ bounds, AsofMode m, AsofCols cols,
            uint32_t* __restrict__ tile_out) {
    __shared__ AsofLDS L;
    const uint32_t tid = threadIdx.x;
    const uint64_t tb = (uint64_t)blockIdx.x * MT_TILE;
    const uint32_t len = (uint32_t)min((uint64_t)MT_TILE, nS - tb);
    const uint64_t Rlo = bounds[2 * blockIdx.x], W = bounds[2 * blockIdx.x + 1] - Rlo;
    stage_s_keys(S, tb, len, L.key);
    const bool staged = stage_r_window(R, Rlo, W, L.rkey);
    __syncthreads();
    const uint32_t i0 = tid * MT_IPT;
    uint32_t matched = 0;
    with_window(staged, L.rkey, R, Rlo, [&](auto rk) {
        matched = asof_partners(rk, Rlo, W, L.key, i0, len, m);
    });
    // the tile's sum shares its barrier with the partners' hand-over, so it
    // is not mat_common.hpp's tile_reduce_store (which brings its own)
    if (tile_out) {
        matched = wave_sum(matched);
        if (lane_id() == 0) L.wsum[tid >> 6] = matched;
    }
    __syncthreads();
    if (tile_out && tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < MT_THREADS / 64; w++) t += L.wsum[w];
        tile_out[blockIdx.x] = t;
    }
    if (!cols.idx && !cols.pay && !cols.key) return;  // the count form
    const bool tuples = cols.pay || cols.key;
    for (uint32_t i = tid; i < len; i += MT_THREADS) {
        const int64_t q = L.key[i];
        MatVal pay = 0, key = 0;
        if (tuples && q >= 0) {
            const Tup r = R[q];
            pay = mat_payload(&r);
            key = (MatVal)tup_key(r);
        }
        if (cols.idx) st_col(cols.idx + tb + i, q);
        if (cols.pay) st_col(cols.pay + tb + i, pay);
        if (cols.key) st_col(cols.key + tb + i, key);
    }
}

void asof_join(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
               uint32_t dir, bool strict, uint64_t tolerance, uint32_t group_shift,
               int64_t* r_index_out, void* r_payload_out, void* r_key_out,
               unsigned long long* matched_dev, hipStream_t st) {
    const AsofCols cols{r_index_out, (MatVal*)r_payload_out, (MatVal*)r_key_out};
    if (nS == 0 || (!cols.idx && !cols.pay && !cols.key && !matched_dev)) return;
    const uint64_t ntiles = (nS + MT_TILE - 1) / MT_TILE;
    // per tile: two window bounds, then (behind them) its matched rows
    uint64_t* bounds = (uint64_t*)ws->scratch("asof_tab", ntiles * (2 * 8 + 4));
    uint32_t* tile_cnt = matched_dev ? (uint32_t*)(bounds + 2 * ntiles) : nullptr;
    const AsofMode m{dir, strict ? 1u : 0u, group_shift, tolerance};
    // nR == 0: every window is empty and no element finds a candidate
    launch_tile_bounds(ws, "k_asof_bounds", k_asof_bounds, ntiles, st, R, nR, S, nS, ntiles,
                       bounds);
    {
        TraceScope ts(ws, "k_asof_tile", st);
        hipLaunchKernelGGL(k_asof_tile, dim3((uint32_t)ntiles), dim3(MT_THREADS), 0, st, R, S, nS,
                           bounds, m, cols, tile_cnt);
        SMJ_CHECK(hipGetLastError());
    }
    if (matched_dev) tile_total(ws, "k_asof_total", tile_cnt, ntiles, matched_dev, st);
}

}  // namespace smj
