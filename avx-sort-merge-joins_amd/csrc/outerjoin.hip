// outerjoin.hip -- left, right and full outer join of two sorted relations
// (smj.h smj_dev_outer_join).  The library's own; the reference has inner
// joins only.
//
// One merge of sorted R and S yields, in ascending order of the union of
// their keys: for a key on both sides its pairs, R-major (materialize.hip's
// order); for a key only in R its R run, one row each (SMJ_OUTER_KEEP_R); for
// a key only in S its S run (SMJ_OUTER_KEEP_S).  An absent side is -1 in the
// index columns and 0 in the value columns.
//
// The passes are those of materialize.hip, over the same S tiles:
//   k_outer_bounds one thread per S tile: the tile's R window and the S extent
//                  of its first and last key runs, as k_mat_bounds, and the R
//                  range the tile OWNS: from the upper bound of the previous
//                  tile's last key (tile 0: R position 0) to the upper bound
//                  of its own last key (last tile: nR).  Every R position is
//                  owned by exactly one tile, and a key whose S run straddles
//                  tiles has its R run owned by the tile where the run starts;
//   k_outer_count  one workgroup per S tile: per S element the R run of its
//                  key [rlo, rhi), searched in the R window staged in LDS (an
//                  owned range beyond the window: searched in global memory).
//                  Per element two row counts: the GAP in front of it -- the
//                  partnerless R tuples between the previous key's R run and
//                  its own, rlo - rhi(previous element), counted at the first
//                  element of a run that starts in the tile -- and its
//                  MATCHES, |R_k| or 1 for a partnerless S element.  After the
//                  last element comes the TAIL, the owned R tuples above the
//                  tile's last key (non-empty only in the last tile);
//   k_mat_scan     materialize.hip's: output bases and work-item bases;
//   k_outer_write  one workgroup per work item of kMatPiece rows: recomputes
//                  the tile's runs, scans the 2 len + 1 gap / match / tail
//                  counts in LDS and writes its piece row-major: per row a
//                  binary search for its entry, then either consecutive R
//                  tuples (a gap: coalesced reads and stores, however long the
//                  run, spread over as many workgroups as it has pieces), one
//                  S tuple, or the pair (off / sc, off % sc) of the key's runs.
// No workgroup waits for another; all counts are 64-bit.
//
// A relation without the other (nS == 0 with KEEP_R, nR == 0 with KEEP_S) is
// an ordered copy, k_outer_side, and needs no host synchronisation.
#include "smj_common.hpp"
#include "smj_internal.hpp"
#include "mat_common.hpp"

namespace smj {

// the output columns (each may be null)
struct OuterCols {
    int64_t* ri;
    int64_t* si;
    MatVal* rp;
    MatVal* sp;
    MatVal* key;
};

// row q: R tuple r and S tuple s, -1 for an absent side (never both)
__device__ __forceinline__ void st_outer(const OuterCols& o, uint64_t q,
                                         const Tup* __restrict__ R,
                                         const Tup* __restrict__ S, int64_t r, int64_t s) {
    if (o.ri) st_col(o.ri + q, r);
    if (o.si) st_col(o.si + q, s);
    MatVal rp = 0, sp = 0, key = 0;
    if (s >= 0 && (o.sp || o.key)) {
        const Tup t = S[s];
        sp = mat_payload(&t);
        key = (MatVal)tup_key(t);
    }
    if (r >= 0 && (o.rp || (o.key && s < 0))) {
        const Tup t = R[r];
        rp = mat_payload(&t);
        if (s < 0) key = (MatVal)tup_key(t);
    }
    if (o.rp) st_col(o.rp + q, rp);
    if (o.sp) st_col(o.sp + q, sp);
    if (o.key) st_col(o.key + q, key);
}

// per tile, 6 words: R window [0], [1]; S start of the first key run [2], S
// end of the last [3]; owned R range [4], [5]
constexpr uint32_t OB_WORDS = 6;

__global__ void __launch_bounds__(256)
k_outer_bounds(const Tup* __restrict__ R, uint64_t nR, const Tup* __restrict__ S,
               uint64_t nS, uint64_t ntiles, uint64_t* __restrict__ bounds) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const TileBounds x = tile_bounds(R, nR, S, nS, t);
    const TupKey rk{R}, sk{S};
    uint64_t os = 0;
    if (x.cont) os = key_search<true>(rk, x.rlo, x.rhi, x.kf);
    else if (x.tb > 0) os = key_search<true>(rk, 0, x.rlo, sk(x.tb - 1));
    uint64_t* b = bounds + OB_WORDS * t;
    x.put(b);
    b[4] = os;
    b[5] = x.te == nS ? nR : x.rhi;
}

// 22.4 KB: 7 workgroups per CU.  The staged R keys are dead once the runs are
// known, and the write pass puts its prefix there.
struct OuterLDS {
    int64_t key[MT_TILE];
    uint64_t rlo[MT_TILE];  // the element's R run [rlo, rhi), positions in R
    uint64_t rhi[MT_TILE];
    uint16_t s0[MT_TILE];   // tile index of the element's run start (0: ends[2])
    uint16_t se[MT_TILE];   // tile index of its run end (len: ends[3])
    union {
        int64_t rkey[MT_RWIN];          // the R window's keys, when it fits
        uint64_t pre[2 * MT_TILE + 1];  // inclusive prefix: gap, matches, ..., tail
    } u;
    uint64_t ends[OB_WORDS];
    uint64_t wsum[MT_THREADS / 64 + 1];
};

// run_walk of mat_common.hpp, keeping both ends of the R run.  Its own copy,
// with outer_tile below for run_tile: through the shared pair k_outer_count
// measured 0.3 to 0.5 % slower at 8 B.  rkey(i) = key
// i of [Rlo, Rhi), position base + i of R
template <class K>
__device__ __forceinline__ void outer_runs(K rkey, uint64_t Rlo, uint64_t Rhi, uint64_t base,
                                           uint32_t i0, uint32_t i1, uint32_t len,
                                           OuterLDS& L) {
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
    uint64_t rlo, rhi = Rlo;
    uint32_t i = i0;
    while (i < i1) {
        const int64_t k = L.key[i];
        uint32_t j = i + 1;
        while (j < i1 && L.key[j] == k) j++;
        if (i != i0) s0 = i;
        rlo = key_gallop<false>(rkey, rhi, Rhi, k);
        rhi = key_gallop<true>(rkey, rlo, Rhi, k);
        const uint32_t e = j < i1 ? j : c;
        for (uint32_t u = i; u < j; u++) {
            L.rlo[u] = base + rlo;
            L.rhi[u] = base + rhi;
            L.s0[u] = (uint16_t)s0;
            L.se[u] = (uint16_t)e;
        }
        i = j;
    }
}

// key runs and R runs of S[tb, tb + len); ends with a barrier
__device__ void outer_tile(const Tup* __restrict__ R, const Tup* __restrict__ S,
                           const uint64_t* __restrict__ bounds, uint64_t t, uint64_t tb,
                           uint32_t len, OuterLDS& L) {
    const uint32_t tid = threadIdx.x;
    if (tid < OB_WORDS) L.ends[tid] = bounds[OB_WORDS * t + tid];
    for (uint32_t i = tid; i < len; i += MT_THREADS) L.key[i] = tup_key(S[tb + i]);
    __syncthreads();
    const uint64_t Rlo = L.ends[0], Rhi = L.ends[1];
    const bool staged = Rhi - Rlo <= MT_RWIN;
    if (staged)
        for (uint32_t i = tid; i < Rhi - Rlo; i += MT_THREADS) L.u.rkey[i] = tup_key(R[Rlo + i]);
    __syncthreads();
    const uint32_t i0 = tid * MT_IPT;
    if (i0 < len) {
        const uint32_t i1 = min(i0 + (uint32_t)MT_IPT, len);
        if (staged) {
            const int64_t* rk = L.u.rkey;
            outer_runs([rk](uint64_t i) { return rk[i]; }, 0, Rhi - Rlo, Rlo, i0, i1, len, L);
        } else {
            outer_runs(TupKey{R}, Rlo, Rhi, 0, i0, i1, len, L);
        }
    }
    __syncthreads();
}

// rows of element u: the gap in front of it and its matches
__device__ __forceinline__ void outer_rows(const OuterLDS& L, uint64_t tb, uint32_t u,
                                           uint32_t keep, uint64_t& gap, uint64_t& match) {
    const uint64_t rc = L.rhi[u] - L.rlo[u];
    match = rc ? rc : (keep & kOuterKeepS) ? 1 : 0;
    gap = 0;
    if (keep & kOuterKeepR) {
        // the first element of a run that starts in this tile
        const bool first = u ? L.s0[u] == u : L.ends[2] == tb;
        if (first) gap = L.rlo[u] - (u ? L.rhi[u - 1] : L.ends[4]);
    }
}

// the owned R tuples above the tile's last key
__device__ __forceinline__ uint64_t outer_tail(const OuterLDS& L, uint32_t len, uint32_t keep) {
    return (keep & kOuterKeepR) ? L.ends[5] - L.rhi[len - 1] : 0;
}

__global__ void __launch_bounds__(MT_THREADS)
k_outer_count(const Tup* __restrict__ R, const Tup* __restrict__ S, uint64_t nS,
              uint32_t keep, const uint64_t* __restrict__ bounds,
              uint64_t* __restrict__ tile_out) {
    __shared__ OuterLDS L;
    const uint64_t tb = (uint64_t)blockIdx.x * MT_TILE;
    const uint32_t len = (uint32_t)min((uint64_t)MT_TILE, nS - tb);
    outer_tile(R, S, bounds, blockIdx.x, tb, len, L);
    const uint32_t i0 = threadIdx.x * MT_IPT;
    uint64_t s = 0;
    for (uint32_t u = i0; u < min(i0 + (uint32_t)MT_IPT, len); u++) {
        uint64_t g, m;
        outer_rows(L, tb, u, keep, g, m);
        s += g + m;
    }
    if (threadIdx.x == 0) s += outer_tail(L, len, keep);
    tile_reduce_store(s, L.wsum, tile_out);
}

__global__ void __launch_bounds__(64)
k_outer_add(unsigned long long* total, unsigned long long n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(total, n);
}

__global__ void __launch_bounds__(MT_THREADS)
k_outer_write(const Tup* __restrict__ R, const Tup* __restrict__ S, uint64_t nS, uint32_t keep,
              const uint64_t* __restrict__ bounds, const uint64_t* __restrict__ cnt,
              const uint64_t* __restrict__ base, const uint64_t* __restrict__ ibase,
              uint64_t ntiles, uint64_t out_cap, OuterCols cols) {
    __shared__ OuterLDS L;
    __shared__ uint64_t sh_t;
    const MatPiece pc = mat_piece(ibase, cnt, base, ntiles, nS, out_cap, &sh_t);
    if (!pc.live) return;
    const uint64_t t = pc.t, q0 = pc.q0, q1 = pc.q1, ob = pc.ob, tb = pc.tb;
    const uint32_t len = pc.len;
    outer_tile(R, S, bounds, t, tb, len, L);
    // inclusive prefix over gap(0), match(0), gap(1), ..., match(len - 1), tail
    const uint32_t i0 = threadIdx.x * MT_IPT;
    const uint32_t i1 = min(i0 + (uint32_t)MT_IPT, len);
    uint64_t g[MT_IPT], m[MT_IPT];
    uint64_t s = 0;
#pragma unroll
    for (uint32_t p = 0; p < MT_IPT; p++) {
        g[p] = m[p] = 0;
        if (i0 + p < i1) outer_rows(L, tb, i0 + p, keep, g[p], m[p]);
        s += g[p] + m[p];
    }
    const uint64_t tail = outer_tail(L, len, keep);
    // the scan's first barrier follows every read of the staged R keys
    uint64_t run = block_scan64(s, L.wsum, nullptr);
#pragma unroll
    for (uint32_t p = 0; p < MT_IPT; p++) {
        if (i0 + p < i1) {
            run += g[p];
            L.u.pre[2 * (i0 + p)] = run;
            run += m[p];
            L.u.pre[2 * (i0 + p) + 1] = run;
            if (i0 + p == len - 1) L.u.pre[2 * len] = run + tail;
        }
    }
    __syncthreads();
    const int64_t first_s0 = (int64_t)L.ends[2], last_se = (int64_t)L.ends[3];
    for (uint64_t q = q0 + threadIdx.x; q < q1; q += MT_THREADS) {
        if (ob + q >= out_cap) break;
        // entry x: the first inclusive prefix above q (q < cnt[t] = pre[2 len])
        const uint32_t x = prefix_pick(L.u.pre, 2 * len, q), j = x >> 1;
        const uint64_t excl = x ? L.u.pre[x - 1] : 0;
        if (!(x & 1)) {
            // a gap ends where element j's R run starts, the tail where the
            // owned range ends
            const uint64_t end = j < len ? L.rlo[j] : L.ends[5];
            const uint64_t r = end - (L.u.pre[x] - q);
            st_outer(cols, ob + q, R, S, (int64_t)r, -1);
            continue;
        }
        const uint64_t rcj = L.rhi[j] - L.rlo[j];
        if (rcj == 0) {
            st_outer(cols, ob + q, R, S, -1, (int64_t)(tb + j));
            continue;
        }
        int64_t s0, se;
        run_extent(L.s0, L.se, j, tb, len, first_s0, last_se, s0, se);
        const uint64_t sc = (uint64_t)(se - s0);
        // the run's pairs are cut into rcj per S element: element j's first
        // is pair (tb + j - s0) * rcj of the run; R-major, R tuple off / sc
        // of the run and S tuple off % sc
        const uint64_t off = (q - excl) + (uint64_t)((int64_t)(tb + j) - s0) * rcj;
        uint64_t d;
        const uint64_t rem = run_pair(off, sc, d);
        st_outer(cols, ob + q, R, S, (int64_t)(L.rlo[j] + d), (int64_t)((uint64_t)s0 + rem));
    }
}

// one relation without the other: row q is tuple q of T (the R side, or with
// s_side the S side), the other side absent
__global__ void __launch_bounds__(256)
k_outer_side(const Tup* __restrict__ T, uint64_t n, int s_side, OuterCols cols) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
        if (s_side) st_outer(cols, q, T, T, -1, (int64_t)q);
        else st_outer(cols, q, T, T, (int64_t)q, -1);
    }
}

// the bounds and count passes
static TileTab outer_count_passes(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S,
                                  uint64_t nS, uint32_t keep, hipStream_t st) {
    const TileTab b = tile_tab(ws, "outer_tab", (nS + MT_TILE - 1) / MT_TILE, OB_WORDS);
    launch_tile_bounds(ws, "k_outer_bounds", k_outer_bounds, b.ntiles, st, R, nR, S, nS,
                       b.ntiles, b.bounds);
    {
        TraceScope ts(ws, "k_outer_count", st);
        hipLaunchKernelGGL(k_outer_count, dim3((uint32_t)b.ntiles), dim3(MT_THREADS), 0, st, R,
                           S, nS, keep, b.bounds, b.cnt);
        SMJ_CHECK(hipGetLastError());
    }
    return b;
}

// the rows when one relation is empty: the other one whole, or none
static uint64_t outer_side_rows(uint64_t nR, uint64_t nS, uint32_t keep) {
    if (nS == 0) return (keep & kOuterKeepR) ? nR : 0;
    return (keep & kOuterKeepS) ? nS : 0;
}

uint64_t outer_join(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                    uint32_t keep, int64_t* r_index_out, int64_t* s_index_out,
                    void* r_payload_out, void* s_payload_out, void* key_out, uint64_t out_cap,
                    hipStream_t st) {
    if (nR == 0 && nS == 0) return 0;
    const OuterCols cols{r_index_out, s_index_out, (MatVal*)r_payload_out,
                         (MatVal*)s_payload_out, (MatVal*)key_out};
    if (!cols.ri && !cols.si && !cols.rp && !cols.sp && !cols.key) out_cap = 0;
    if (nR == 0 || nS == 0) {
        const uint64_t total = outer_side_rows(nR, nS, keep);
        const uint64_t n = total < out_cap ? total : out_cap;
        if (n) {
            TraceScope ts(ws, "k_outer_side", st);
            const uint64_t blocks = (n + 255) / 256;
            hipLaunchKernelGGL(k_outer_side, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)),
                               dim3(256), 0, st, nS ? S : R, n, nS ? 1 : 0, cols);
            SMJ_CHECK(hipGetLastError());
        }
        return total;
    }
    const TileTab b = outer_count_passes(ws, R, nR, S, nS, keep, st);
    const MatFinish f = mat_finish(ws, "outer_tot_h", b, out_cap, st);
    if (f.launch) {
        TraceScope ts(ws, "k_outer_write", st);
        hipLaunchKernelGGL(k_outer_write, dim3((uint32_t)f.launch), dim3(MT_THREADS), 0, st, R, S,
                           nS, keep, b.bounds, b.cnt, b.base, b.ibase, b.ntiles, out_cap, cols);
        SMJ_CHECK(hipGetLastError());
    }
    return f.total;
}

void outer_join_count(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                      uint32_t keep, unsigned long long* count_dev, hipStream_t st) {
    if (nR == 0 || nS == 0) {
        const uint64_t total = outer_side_rows(nR, nS, keep);
        if (total) {
            hipLaunchKernelGGL(k_outer_add, dim3(1), dim3(64), 0, st, count_dev,
                               (unsigned long long)total);
            SMJ_CHECK(hipGetLastError());
        }
        return;
    }
    const TileTab b = outer_count_passes(ws, R, nR, S, nS, keep, st);
    tile_total(ws, nullptr, b.cnt, b.ntiles, count_dev, st);
}

}  // namespace smj
