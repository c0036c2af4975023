// bandjoin.hip -- band join of two sorted relations (smj.h smj_dev_band_join):
// every pair (r, s) with s.key + lo <= r.key <= s.key + hi.  The library's
// own; the reference has equality joins only.
//
// In sorted R the partners of one S tuple are one contiguous range
// R[lb, ub): lb the first key >= s.key + lo, ub the first key > s.key + hi,
// both non-decreasing along sorted S.  The sums saturate at the ends of int64
// and an S tuple whose band lies wholly outside int64 has no partner (a
// predicate without wrap-around).  The output is S-major: for each S tuple in
// sorted order, its R range in sorted order.
//
// The passes are those of materialize.hip, over the same tiles:
//   k_band_bounds one thread per S tile: the tile's R window, from the lower
//                 bound of its first element to the upper bound of its last;
//   k_band_count  one workgroup per S tile: the tile's keys and (when it
//                 fits) the window's keys staged in LDS; per element the two
//                 bounds, each galloping on from the previous element's;
//                 leaves (start in the window, length) per element and the
//                 tile's sum;
//   k_mat_scan    materialize.hip's: output bases and work-item bases;
//   k_band_write  one workgroup per work item of kMatPiece outputs: the
//                 tile's inclusive prefix of lengths in LDS; per output a
//                 binary search for its element j, then R[window + start_j +
//                 (q - excl_j)] and S[tb + j] into the columns.  Consecutive
//                 outputs of an element read consecutive R tuples, and one
//                 element with a huge range spreads over many workgroups.
// The stored entries are 32-bit; a tile whose window spans 2^kBandWideBits R
// tuples or more stores none and the write pass searches again.
#include "smj_common.hpp"
#include "smj_internal.hpp"
#include "mat_common.hpp"

namespace smj {

// windows of 2^kBandWideBits tuples and more are searched again by the write
// pass (0: every window -- the variant DESIGN.md section 7 measures)
#ifndef SMJ_BAND_WIDE_BITS
#define SMJ_BAND_WIDE_BITS 32
#endif
constexpr uint32_t kBandWideBits = SMJ_BAND_WIDE_BITS;
static_assert(kBandWideBits <= 32, "the stored entries are 32-bit");

__device__ __forceinline__ bool band_wide(uint64_t w) { return (w >> kBandWideBits) != 0; }

// the output columns (the key columns may be null)
struct BandCols {
    MatVal* r;
    MatVal* s;
    MatVal* rkey;
    MatVal* skey;
};

// per tile: its R window [lb(first key + lo), ub(last key + hi))
__global__ void __launch_bounds__(256)
k_band_bounds(const Tup* __restrict__ R, uint64_t nR, const Tup* __restrict__ S,
              uint64_t nS, int64_t lo, int64_t hi, uint64_t ntiles,
              uint64_t* __restrict__ bounds) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const uint64_t tb = t * MT_TILE;
    const uint64_t te = min(tb + MT_TILE, nS);
    const TupKey rk{R}, sk{S};
    int over;
    const int64_t a = sat_add(sk(tb), lo, over), b = sat_add(sk(te - 1), hi, over);
    const uint64_t rlo = key_search<false>(rk, 0, nR, a);
    bounds[2 * t + 0] = rlo;
    bounds[2 * t + 1] = key_search<true>(rk, rlo, nR, b);  // b >= a
}

struct BandLDS {
    int64_t key[MT_TILE];
    int64_t rkey[MT_RWIN];  // the R window's keys, when it fits
    uint64_t wsum[MT_THREADS / 64 + 1];
};

// ranges of the thread's elements [i0, i0 + MT_IPT) of a tile of len: start
// in the window of W keys (K(i) = key i of it) and length
template <class K>
__device__ __forceinline__ void band_ranges(K rkey, uint64_t W, const int64_t* skey,
                                            uint32_t i0, uint32_t len, int64_t lo,
                                            int64_t hi, uint64_t (&start)[MT_IPT],
                                            uint64_t (&cnt)[MT_IPT]) {
    uint64_t lb = 0, ub = 0;
#pragma unroll
    for (uint32_t p = 0; p < MT_IPT; p++) {
        start[p] = cnt[p] = 0;
        if (i0 + p < len) {
            int oa, ob;
            const int64_t a = sat_add(skey[i0 + p], lo, oa);
            const int64_t b = sat_add(skey[i0 + p], hi, ob);
            lb = key_gallop<false>(rkey, lb, W, a);
            ub = key_gallop<true>(rkey, max(ub, lb), W, b);  // b >= a
            start[p] = lb;
            cnt[p] = (oa > 0 || ob < 0) ? 0 : ub - lb;  // the band outside int64
        }
    }
}

// the ranges of S[tb, tb + len) in the window R[Rlo, Rlo + W); every thread
// of the workgroup calls it
__device__ __forceinline__ void band_tile(const Tup* __restrict__ R,
                                          const Tup* __restrict__ S, uint64_t Rlo,
                                          uint64_t W, uint64_t tb, uint32_t len, int64_t lo,
                                          int64_t hi, BandLDS& L, uint64_t (&start)[MT_IPT],
                                          uint64_t (&cnt)[MT_IPT]) {
    // mat_common.hpp's stage_s_keys / stage_r_window / with_window written out:
    // through the helpers k_band_count took 32 VGPRs for 30 and measured 0.5 %
    // slower
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < len; i += MT_THREADS) L.key[i] = tup_key(S[tb + i]);
    const bool staged = W <= MT_RWIN;
    if (staged)
        for (uint32_t i = tid; i < W; i += MT_THREADS) L.rkey[i] = tup_key(R[Rlo + i]);
    __syncthreads();
    const uint32_t i0 = tid * MT_IPT;
    if (staged) band_ranges(LdsKey{L.rkey}, W, L.key, i0, len, lo, hi, start, cnt);
    else band_ranges(TupKey{R + Rlo}, W, L.key, i0, len, lo, hi, start, cnt);
}

// ent null: a count-only call, nothing will read the entries
__global__ void __launch_bounds__(MT_THREADS)
k_band_count(const Tup* __restrict__ R, const Tup* __restrict__ S, uint64_t nS, int64_t lo,
             int64_t hi, const uint64_t* __restrict__ bounds, uint64_t* __restrict__ tile_out,
             uint2* __restrict__ ent) {
    __shared__ BandLDS L;
    const uint64_t tb = (uint64_t)blockIdx.x * MT_TILE;
    const uint32_t len = (uint32_t)min((uint64_t)MT_TILE, nS - tb);
    const uint64_t Rlo = bounds[2 * blockIdx.x], W = bounds[2 * blockIdx.x + 1] - Rlo;
    uint64_t start[MT_IPT], cnt[MT_IPT];
    band_tile(R, S, Rlo, W, tb, len, lo, hi, L, start, cnt);
    const uint32_t i0 = threadIdx.x * MT_IPT;
    uint64_t s = 0;
#pragma unroll
    for (uint32_t p = 0; p < MT_IPT; p++) {
        s += cnt[p];
        if (ent && !band_wide(W) && i0 + p < len)
            ent[tb + i0 + p] = make_uint2((uint32_t)start[p], (uint32_t)cnt[p]);
    }
    tile_reduce_store(s, L.wsum, tile_out);
}

__global__ void __launch_bounds__(MT_THREADS)
k_band_write(const Tup* __restrict__ R, const Tup* __restrict__ S, uint64_t nS, int64_t lo,
             int64_t hi, const uint64_t* __restrict__ bounds, const uint2* __restrict__ ent,
             const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ base,
             const uint64_t* __restrict__ ibase, uint64_t ntiles, uint64_t out_cap,
             BandCols cols) {
    __shared__ BandLDS L;
    __shared__ uint64_t pre[MT_TILE];  // inclusive prefix of the range lengths
    __shared__ uint64_t beg[MT_TILE];  // range starts in the window
    __shared__ uint64_t sh_t;
    const MatPiece pc = mat_piece(ibase, cnt, base, ntiles, nS, out_cap, &sh_t);
    if (!pc.live) return;
    const uint64_t t = pc.t, q0 = pc.q0, q1 = pc.q1, ob = pc.ob, tb = pc.tb;
    const uint32_t len = pc.len;
    const uint64_t Rlo = bounds[2 * t], W = bounds[2 * t + 1] - Rlo;
    const uint32_t i0 = threadIdx.x * MT_IPT;
    uint64_t start[MT_IPT], c[MT_IPT];
    if (band_wide(W)) {  // uniform over the workgroup
        band_tile(R, S, Rlo, W, tb, len, lo, hi, L, start, c);
    } else {
#pragma unroll
        for (uint32_t p = 0; p < MT_IPT; p++) {
            const uint2 e = i0 + p < len ? ent[tb + i0 + p] : make_uint2(0, 0);
            start[p] = e.x;
            c[p] = e.y;
        }
    }
    uint64_t s = 0;
#pragma unroll
    for (uint32_t p = 0; p < MT_IPT; p++) s += c[p];
    uint64_t run = block_scan64(s, L.wsum, nullptr);
#pragma unroll
    for (uint32_t p = 0; p < MT_IPT; p++) {
        run += c[p];
        if (i0 + p < len) {
            pre[i0 + p] = run;
            beg[i0 + p] = start[p];
        }
    }
    __syncthreads();
    const Tup* rw = R + Rlo;
    for (uint64_t q = q0 + threadIdx.x; q < q1; q += MT_THREADS) {
        if (ob + q >= out_cap) break;
        // element j: the first inclusive prefix above q (q < cnt[t] = pre[len - 1])
        const uint32_t j = prefix_pick(pre, len - 1, q);
        const uint64_t excl = j ? pre[j - 1] : 0;
        const Tup r = rw[beg[j] + (q - excl)];
        const Tup sj = S[tb + j];
        st_col(cols.r + ob + q, mat_payload(&r));
        st_col(cols.s + ob + q, mat_payload(&sj));
        if (cols.rkey) st_col(cols.rkey + ob + q, (MatVal)tup_key(r));
        if (cols.skey) st_col(cols.skey + ob + q, (MatVal)tup_key(sj));
    }
}

// the bounds and count passes; ent null: no entries are kept
static TileTab band_count_passes(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S,
                                 uint64_t nS, int64_t lo, int64_t hi, uint2* ent,
                                 hipStream_t st) {
    const TileTab b = tile_tab(ws, "band_tab", (nS + MT_TILE - 1) / MT_TILE, 2);
    launch_tile_bounds(ws, "k_band_bounds", k_band_bounds, b.ntiles, st, R, nR, S, nS, lo, hi,
                       b.ntiles, b.bounds);
    {
        TraceScope ts(ws, "k_band_count", st);
        hipLaunchKernelGGL(k_band_count, dim3((uint32_t)b.ntiles), dim3(MT_THREADS), 0, st, R,
                           S, nS, lo, hi, b.bounds, b.cnt, ent);
        SMJ_CHECK(hipGetLastError());
    }
    return b;
}

uint64_t band_join(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                   int64_t lo, int64_t hi, void* r_out, void* s_out, void* r_key_out,
                   void* s_key_out, uint64_t out_cap, hipStream_t st) {
    if (lo > hi || nR == 0 || nS == 0) return 0;
    uint2* ent = out_cap ? (uint2*)ws->scratch("band_ent", nS * sizeof(uint2)) : nullptr;
    const TileTab b = band_count_passes(ws, R, nR, S, nS, lo, hi, ent, st);
    const MatFinish f = mat_finish(ws, "band_tot_h", b, out_cap, st);
    if (f.launch) {
        const BandCols cols{(MatVal*)r_out, (MatVal*)s_out, (MatVal*)r_key_out,
                            (MatVal*)s_key_out};
        TraceScope ts(ws, "k_band_write", st);
        hipLaunchKernelGGL(k_band_write, dim3((uint32_t)f.launch), dim3(MT_THREADS), 0, st, R, S,
                           nS, lo, hi, b.bounds, ent, b.cnt, b.base, b.ibase, b.ntiles, out_cap,
                           cols);
        SMJ_CHECK(hipGetLastError());
    }
    return f.total;
}

void band_join_count(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                     int64_t lo, int64_t hi, unsigned long long* count_dev, hipStream_t st) {
    if (lo > hi || nR == 0 || nS == 0) return;
    const TileTab b = band_count_passes(ws, R, nR, S, nS, lo, hi, nullptr, st);
    tile_total(ws, nullptr, b.cnt, b.ntiles, count_dev, st);
}

}  // namespace smj
