// smj_internal.hpp -- host-side internal interfaces between the .hip units.
#pragma once
#include <sched.h>

#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_ext.h>

#include "smj_common.hpp"

namespace smj {

constexpr uint32_t kNarrowDigitBits = 12;  // widest digit of a single pass
// widest level-2 digit (groups per bucket): k_preft stages 64 prefix rows of
// 2^kMaxD2 + 1 entries in LDS
constexpr uint32_t kMaxD2 = 10;

// reference partition digit (runtime mask/shift), see smj_common.hpp
typedef RefDigit Digit32;

// wave-uniform 32/64-bit values into SGPRs
__device__ __forceinline__ uint32_t uniform32(uint32_t x) {
    return __builtin_amdgcn_readfirstlane(x);
}
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(x >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((uint32_t)x);
}

// level-1 digit of a range plan held by value (in SGPRs)
struct PlanDigitV {
    RangePlan p;
    __device__ __forceinline__ uint32_t operator()(const Tup& t) const {
        return plan_d1(p, plan_rel(p, tup_key(t)));
    }
};

// level-1 digit of a device-resident range plan.  Kernels call load() once:
// the plan is read a single time instead of at every digit (the output
// stores may alias it, so the compiler would reload it).
struct PlanDigit1 {
    const RangePlan* plan;
    __device__ __forceinline__ PlanDigitV load() const {
        RangePlan q = *plan;
        PlanDigitV v;
        v.p.base = (int64_t)uniform64((uint64_t)q.base);
        v.p.span = uniform64(q.span);
        v.p.D1 = uniform32(q.D1);
        v.p.D2 = uniform32(q.D2);
        v.p.D3 = uniform32(q.D3);
        v.p.s1 = uniform32(q.s1);
        v.p.s2 = uniform32(q.s2);
        v.p.s3 = uniform32(q.s3);
        return v;
    }
};

// Grow-only named device scratch.  Reallocation frees the old buffer with
// hipFree (which synchronises), so it only happens on warm-up calls.
#ifndef SMJ_SPIN_WAIT
#define SMJ_SPIN_WAIT 1  // Workspace::wait_stream polls an event (0: a lab build's stream sync)
#endif
struct Workspace {
    // layouts this workspace's sorts and joins may not use
    // (smj_workspace_set_layouts, SMJ_LAYOUT_* in smj.h)
    uint32_t layouts_off = 0;
    // What the last joins and sorts of a few shapes (relation sizes) learnt
    // about their payloads (ShapeHint, layout_policy.hpp), least recently
    // used first out, so a caller alternating shapes on one workspace (sort R,
    // sort S, join R and S) keeps every shape's hint
    ShapeHint hints[8];
    uint64_t hint_clock = 0;
    ShapeHint& hint_for(uint64_t shape) {
        ShapeHint* victim = &hints[0];
        for (ShapeHint& h : hints) {
            if (h.shape == shape) {
                h.used = ++hint_clock;
                return h;
            }
            if (h.used < victim->used) victim = &h;
        }
        *victim = ShapeHint();
        victim->shape = shape;
        victim->used = ++hint_clock;
        return *victim;
    }
    int last_layout = -1;  // smj_workspace_last_layout (SMJ_LAYOUT_USED_*)
    // smj_workspace_force_ballot_ranks: the stable partition chooses as on a
    // device whose LDS atomics fail the lane-order self-check
    // (partition_policy.hpp); smj_workspace_last_scatter: SMJ_SCATTER_* of
    // what the last stable_partition launched
    bool force_ballot_ranks = false;
    uint32_t last_scatter = 0;
    // smj_workspace_skew_stats: what the skew path of the last completed
    // bucket pass did, in the order of smj_skew_stats (smj.h); host values the
    // pass holds anyway
    struct SkewStats {
        uint32_t tpl = 0, queued = 0, empty = 0, small = 0, large = 0, items = 0, inexact = 0,
                 unordered = 0, resorted = 0, recounted = 0;
    };
    SkewStats skew;
    bool skew_valid = false;
    // smj_workspace_merge_stats: what the last multiway_merge decided (host
    // values: form SMJ_MERGE_* of smj.h, runs, bucket bits) and the overflow
    // queue its one-pass form used (word 0, the queue's length, is read by the
    // accessor, not by the merge)
    struct MergeStats {
        uint32_t form = 0, k = 0, D = 0;
        const unsigned int* queue = nullptr;
    };
    MergeStats merge;
    bool merge_valid = false;
    std::map<std::string, std::pair<void*, size_t>> bufs;
    std::map<std::string, std::pair<void*, size_t>> pinned;
    // the k-way merge's run table as last uploaded, and where (a repeated
    // merge of the same runs skips the upload)
    std::vector<unsigned char> km_last;
    const void* km_last_dev = nullptr;
    hipEvent_t ev[8] = {};
    bool ev_init = false;
    float phase_ms[5] = {0, 0, 0, 0, 0};

    void* scratch(const char* name, size_t bytes) {
        if (bytes == 0) bytes = 16;
        auto it = bufs.find(name);
        if (it != bufs.end() && it->second.second >= bytes)
            return it->second.first;
        if (it != bufs.end()) SMJ_CHECK(hipFree(it->second.first));
        void* p = nullptr;
        size_t cap = bytes + bytes / 8;
        SMJ_CHECK(hipMalloc(&p, cap));
        bufs[name] = {p, cap};
        return p;
    }
    void* host_pinned(const char* name, size_t bytes) {
        if (bytes == 0) bytes = 16;
        auto it = pinned.find(name);
        if (it != pinned.end() && it->second.second >= bytes)
            return it->second.first;
        if (it != pinned.end()) SMJ_CHECK(hipHostFree(it->second.first));
        void* p = nullptr;
        SMJ_CHECK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        pinned[name] = {p, bytes};
        return p;
    }
    // Rings of pinned staging slots for host-built tables that are uploaded
    // stream-ordered before a launch: a slot is rewritten only after the copy
    // that used it kNRing uploads ago has finished (its event), so
    // consecutive launches never wait for the stream to drain.
    static constexpr uint32_t kNRing = 8;
    struct RingSlot {
        void* p = nullptr;
        size_t cap = 0;
        hipEvent_t ev = nullptr;
        bool used = false;
    };
    std::map<std::string, std::pair<std::vector<RingSlot>, uint32_t>> rings;
    void* ring_acquire(const char* name, size_t bytes, uint32_t* slot) {
        auto& r = rings[name];
        if (r.first.empty()) r.first.resize(kNRing);
        const uint32_t i = r.second++ % kNRing;
        RingSlot& s = r.first[i];
        if (s.used) SMJ_CHECK(hipEventSynchronize(s.ev));
        if (s.cap < bytes) {
            if (s.p) SMJ_CHECK(hipHostFree(s.p));
            SMJ_CHECK(hipHostMalloc(&s.p, bytes ? bytes : 16, hipHostMallocDefault));
            s.cap = bytes;
        }
        if (!s.ev) SMJ_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
        *slot = i;
        return s.p;
    }
    // after the hipMemcpyAsync that reads the slot
    void ring_release(const char* name, uint32_t slot, hipStream_t st) {
        RingSlot& s = rings[name].first[slot];
        SMJ_CHECK(hipEventRecord(s.ev, st));
        s.used = true;
    }
    // The host's wait for a stream (the per-call synchronisation that reads
    // the status flags): an event behind the stream's work, polled with
    // hipEventQuery (busy wait) instead of hipStreamSynchronize's blocking
    // wait, which wakes the thread several microseconds after the work ends.
    hipEvent_t wait_ev = nullptr;
    void wait_stream(hipStream_t st) {
#if SMJ_SPIN_WAIT
        if (!wait_ev) SMJ_CHECK(hipEventCreateWithFlags(&wait_ev, hipEventDisableTiming));
        SMJ_CHECK(hipEventRecord(wait_ev, st));
        // spin for a bounded time (the short waits of a join step end in a
        // few microseconds); past it, yield the core and then block, so long
        // sorts and merges do not hold a host core at 100 %
        hipError_t e;
        const auto t0 = std::chrono::steady_clock::now();
        while ((e = hipEventQuery(wait_ev)) == hipErrorNotReady) {
            const auto dt = std::chrono::steady_clock::now() - t0;
            if (dt > std::chrono::microseconds(200)) {
                e = hipEventSynchronize(wait_ev);
                break;
            }
            if (dt > std::chrono::microseconds(50)) sched_yield();
        }
        SMJ_CHECK(e);
#else
        SMJ_CHECK(hipStreamSynchronize(st));
#endif
    }
    void events() {
        if (!ev_init) {
            for (auto& e : ev) SMJ_CHECK(hipEventCreate(&e));
            ev_init = true;
        }
    }

    // per-kernel event trace (bench.py's roofline needs each kernel's own
    // duration over the timed region); off unless smj_trace_enable()
    struct TraceRec {
        const char* name;
        hipEvent_t a, b;
    };
    bool trace_on = false;
    std::string trace_only;  // non-empty: trace this kernel name alone
    std::vector<TraceRec> trace;
    size_t trace_n = 0;
    bool traced(const char* name) const {
        return trace_on && (trace_only.empty() || trace_only == name);
    }
    int trace_begin(const char* name, hipStream_t st) {
        if (!traced(name)) return -1;
        if (trace_n == trace.size()) {
            TraceRec r;
            SMJ_CHECK(hipEventCreate(&r.a));
            SMJ_CHECK(hipEventCreate(&r.b));
            trace.push_back(r);
        }
        trace[trace_n].name = name;
        SMJ_CHECK(hipEventRecord(trace[trace_n].a, st));
        return (int)trace_n++;
    }
    void trace_end(int idx, hipStream_t st) {
        if (idx >= 0) SMJ_CHECK(hipEventRecord(trace[idx].b, st));
    }
    // a trace record whose events the runtime stamps at the kernel's own start
    // and end (hipExtLaunchKernelGGL): no event-record gap around short kernels
    bool trace_ext(const char* name, hipEvent_t* a, hipEvent_t* b) {
        if (!traced(name)) return false;
        if (trace_n == trace.size()) {
            TraceRec r;
            SMJ_CHECK(hipEventCreate(&r.a));
            SMJ_CHECK(hipEventCreate(&r.b));
            trace.push_back(r);
        }
        trace[trace_n].name = name;
        *a = trace[trace_n].a;
        *b = trace[trace_n].b;
        trace_n++;
        return true;
    }

    ~Workspace() {
        for (auto& r : trace) {
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        for (auto& kv : bufs) (void)hipFree(kv.second.first);
        for (auto& kv : pinned) (void)hipHostFree(kv.second.first);
        if (ev_init)
            for (auto& e : ev) (void)hipEventDestroy(e);
    }
};

struct TraceScope {
    Workspace* ws;
    hipStream_t st;
    int idx;
    TraceScope(Workspace* w, const char* name, hipStream_t s)
        : ws(w), st(s), idx(w ? w->trace_begin(name, s) : -1) {}
    ~TraceScope() {
        if (ws) ws->trace_end(idx, st);
    }
};

// One traced kernel launch: with tracing on, the trace events are stamped by
// the launch itself (kernel-exact, like the profiler's kernel trace).
template <typename... KArgs, typename... Args>
inline void traced_launch(Workspace* ws, const char* name, void (*kernel)(KArgs...),
                          dim3 grid, dim3 block, uint32_t shmem, hipStream_t st,
                          Args... args) {
    hipEvent_t a, b;
    if (ws && ws->trace_ext(name, &a, &b))
        hipExtLaunchKernelGGL(kernel, grid, block, shmem, st, a, b, 0u, (KArgs)args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, shmem, st, (KArgs)args...);
}

// ---- refgen.hip : the reference's rand()-driven generators, bit-exact
uint32_t glibc_rand_at(uint32_t seed, uint64_t k);  // the k-th rand() after srand(seed)
void gen_nonunique_ref(Workspace* ws, Tup* out, uint64_t n, uint64_t first, uint64_t total,
                       int64_t maxid, uint32_t seed, uint64_t skip, hipStream_t st);
void gen_zipf_ref(Workspace* ws, Tup* out, uint64_t n, uint64_t first, uint64_t maxid,
                  double theta, uint32_t seed, uint64_t skip, hipStream_t st);

// ---- exchange.hip : the multi-GPU exchange's tables
void xsend(const int64_t* start, const int64_t* cnt, const unsigned int* flags, uint32_t F,
           uint32_t K, uint32_t G, uint32_t U, int64_t* msg, int64_t* chunk, hipStream_t st);
void xrecv(const int64_t* msg, const int64_t* chunk, uint32_t G, uint32_t rank, uint32_t mine,
           uint32_t K, uint32_t nb, uint64_t cap, int64_t* tstart, int64_t* tcnt,
           int64_t* summary, hipStream_t st);
// exact partition (hist) -> start/cnt tables of K shards, shard 0 used (F <= 1024)
void hist_tables(const int64_t* hist, uint32_t F, uint32_t K, int64_t* start, int64_t* cnt,
                 hipStream_t st);

// ---- partition.hip
void stable_partition(Workspace* ws, const Tup* in, uint64_t n, Tup* out,
                      const Digit32& dig, uint32_t dbits, int padded,
                      int64_t* hist_out, int64_t* off_out, hipStream_t st);
void plan_partition(Workspace* ws, const Tup* in, uint64_t n, Tup* out,
                    const RangePlan* plan_dev, uint32_t dbits,
                    uint64_t* starts_dev, int64_t* hist_out, hipStream_t st);
#ifdef KEY_8B
void plan_partition_packed(Workspace* ws, const Tup* in, uint64_t n, uint64_t* out,
                           const RangePlan* plan_dev, const RangePlan& pack_plan,
                           uint32_t dbits, uint64_t* starts_dev, int64_t* hist_out,
                           unsigned int* pack_bad, hipStream_t st);
#endif
// sampled level-1 partition (join): regions with slack, no histogram pass
uint64_t sampled_capacity(uint64_t n, uint32_t dbits);
// every partition is kShards segments: seg_start/seg_cnt[d * kShards + q]
#ifndef SMJ_SHARDS
#define SMJ_SHARDS 8
#endif
constexpr uint32_t kShards = SMJ_SHARDS;
// Sampled level-1 partition of nrel (1 or 2) relations in shared launches.
// out[r] holds sampled_capacity() elements of `lay` for host_plan (needed by
// every layout but Tuples; Words and P96: 16-byte tuples only), P48 and P96 in
// two planes of `pstride` elements.  When `bad` is given, *bad is OR-ed with
// kBadPayload* (a payload does not pack) and kBadRange (a key lies outside
// host_plan): packed elements need both, tuples are range-checked when the
// plan was guessed.  `sample` = nrel * 2^dbits counters, zeroed by the caller
// (k_join_begin); exact (Tuples, Words): kShards times as many, counted.
void sampled_partition(Workspace* ws, int nrel, const Tup* const* in, const uint64_t* n,
                       void* const* out, const RangePlan* plan_dev, uint32_t dbits,
                       unsigned int* sample, uint64_t* const* starts_dev,
                       int64_t* const* hist_out, uint64_t* const* seg_start,
                       int64_t* const* seg_cnt, unsigned int* flag_dev, hipStream_t st,
                       Layout lay, const RangePlan* host_plan, unsigned int* bad,
                       uint64_t pstride = 0, bool exact = false);
void hist_memcpy(Workspace* ws, const Tup* in, uint64_t n, Tup* out,
                 uint32_t dbits, hipStream_t st);
// lane order of LDS atomic returns (k_scatter_swp's ranks): violations, 0 expected
uint64_t lds_order_selfcheck(Workspace* ws, hipStream_t st);

// ---- bucketsort.hip : MSD bucket sort (+ fused merge-join count)
extern const uint32_t kGroupTarget;  // expected tuples per group of the plan
extern const uint32_t kTileTuples;   // bucket-size unit of the plan (8192)
extern const uint32_t kGroupD3Max;   // widest level-3 digit of the group pass
struct BucketSortArgs {
    // level-1 partitioned relation(s): bucket b occupies
    // [bstart[b], bstart[b] + bcount[b]) of `part`.
    const void* part[2];        // elements of `layout`
    const uint64_t* bstart[2];  // device, nbuckets
    const int64_t* bcount[2];   // device, nbuckets
    // optional (sampled partition): bucket b = kShards segments
    // [seg_start[b*kShards+q], + seg_cnt[...]) inside its region
    const uint64_t* seg_start[2] = {nullptr, nullptr};
    const int64_t* seg_cnt[2] = {nullptr, nullptr};
    uint32_t nseg = kShards;    // segments per bucket (the exchange: one per source GPU)
    void* tmp[2];               // same size as part (tile-local pass output)
    Tup* out[2];                // sorted output, bucket b at ostart[b]
    uint64_t n[2];
    int nrel;                   // 1 = sort only, 2 = R and S + join count
    uint32_t nbuckets;          // 1 << D1
    const RangePlan* plan_dev;
    unsigned long long* count_dev;  // join count (nrel == 2), accumulated
    const unsigned int* part_flag = nullptr;  // sampled partition overflowed?
    // the plan, when the host computed it (key-range hints): with a sampled
    // partition the bucket pass then runs without a mid-pipeline host sync
    const RangePlan* host_plan = nullptr;
    // what part/tmp hold (all but Tuples: packed for host_plan).  P48 (lo
    // uint32, then hi uint16) and P96: two planes of pstride[r] elements each
    Layout layout = Layout::Tuples;
    uint64_t pstride[2] = {0, 0};
    // optional 4-word block zeroed by the caller: [0] = part_flag, [1] =
    // pack_bad, [2] = the skew queue length (read back in one copy)
    unsigned int* status = nullptr;
    const unsigned int* pack_bad = nullptr;  // set by the partition: not packable
    // host copy of status words [0] and [1] after a false return (why the
    // attempt was void: overflow, kBadPayload / kBadRange)
    uint32_t* status_out = nullptr;
    // the 32-bit digit fast path of the tile and group passes (keys outside
    // the plan range only in the first and the last bucket); the segmented
    // join turns it off for tuples (a caller's key outside its range could sit
    // in the last non-empty bucket instead)
    bool digit_fast = true;
    // which stages run (bucket_sort_nosync; segmented joins): bit r = the
    // tile stage (tile numbering, tile pass, prefix table) of relation r,
    // bit 2 = the group pass and the one synchronisation.  A later call runs
    // the stages an earlier one left out, with the same arguments: the
    // multi-GPU join sorts R's tiles while S's rows are still in flight.
    uint32_t stage = 7;
    hipEvent_t ev_tile = nullptr;   // optional phase markers
    hipEvent_t ev_bucket = nullptr;
    hipEvent_t ev_ovf = nullptr;
};
// Runs the tile pass and the group pass; handles overflowing groups (skew)
// with the merge-sort fallback.  Synchronises `st` twice: once for the bucket
// counts (launch sizes) and once for the overflow count.
// Returns false (and does nothing) when a->part_flag reports an overflowed
// sampled partition: the caller repeats the exact partition.
bool bucket_sort(Workspace* ws, const BucketSortArgs& a, hipStream_t st);
// smj_tilepass_occupancy (smj.h) of the 48-bit planes' kernel or the 32-bit
// words' (-1 for the other layouts)
int tilepass_occupancy(Layout lay, uint32_t d2);

// plan selection from a device sample (writes plan_dev)
// (D2 is the size-preferred level-2 width, D2cap the widest the plan may use
// to make the last digit exact)
void plan_from_sample(Workspace* ws, const Tup* const* rels,
                      const uint64_t* ns, int nrel, uint32_t D1, uint32_t D2,
                      uint32_t D2cap, int64_t hint_min, int64_t hint_max,
                      RangePlan* plan_dev, hipStream_t st);

// ---- mergesort.hip : general segmented merge sort + merge path kernels
void segmented_sort(Workspace* ws, Tup* data, const uint64_t* seg_off_host,
                    const uint64_t* seg_len_host, uint32_t nseg, hipStream_t st);
void merge2(Workspace* ws, const Tup* a, uint64_t na, const Tup* b, uint64_t nb, Tup* out,
            hipStream_t st);
void merge_join_count(const Tup* r, uint64_t nr, const Tup* s, uint64_t ns,
                      unsigned long long* count_dev, hipStream_t st);
// k independent merge-join counts (host arrays), one launch
void merge_join_count_batch(Workspace* ws, const Tup* const* r, const uint64_t* nr,
                            const Tup* const* s, const uint64_t* ns, uint32_t k,
                            unsigned long long* count_dev, hipStream_t st);
// Workspace::merge.form (SMJ_MERGE_* of smj.h; capi.hip asserts the match)
constexpr uint32_t kMergeNone = 0, kMergeBuckets = 1, kMergeTree = 2;
void multiway_merge(Workspace* ws, const Tup* const* runs_host,
                    const uint64_t* lens_host, uint32_t k, Tup* out,
                    hipStream_t st);
// the 2-way merge-path tree only (the m-pass join's multi-pass merging)
void multiway_merge_tree(Workspace* ws, const Tup* const* runs_host,
                         const uint64_t* lens_host, uint32_t k, Tup* out,
                         hipStream_t st);

// ---- materialize.hip : merge-join output tuples (sorted R and S)
// Writes the first min(total, out_cap) output tuples and returns the total
// (synchronises `st` once, for the launch size of the write pass).
uint64_t materialize(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S,
                     uint64_t nS, Tup* out, uint64_t out_cap, hipStream_t st);
// The join index: for output position q of materialize(), the payloads of
// the matching R and S tuples (and the key, unless key_out is null) as
// columns of the ABI's value_t / intkey_t.  The same capacity and
// synchronisation rules.
uint64_t join_pairs(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                    void* r_out, void* s_out, void* key_out, uint64_t out_cap,
                    hipStream_t st);
// The S tuples whose key occurs in R (anti: does not occur), in sorted order.
uint64_t semi_join(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                   Tup* out, uint64_t out_cap, int anti, hipStream_t st);
// The scan between the count pass and the write pass (traced as k_mat_scan):
// from the output counts of ntiles S tiles, the tiles' output bases and the
// bases of their work items (pieces of kMatPiece outputs, mat_common.hpp),
// both exclusive; tot[0..1] = the outputs and the work items in all.
void mat_scan(Workspace* ws, const uint64_t* cnt, uint64_t ntiles, uint64_t* base,
              uint64_t* ibase, uint64_t* tot, hipStream_t st);
// The per-tile tables of the count -> scan -> write operators, carved from one
// scratch buffer of ((3 + bounds_words) ntiles + 2) * 8 + extra_bytes bytes:
// cnt, base, ibase (ntiles each), bounds (bounds_words a tile), tot (2 words);
// the extra bytes, an operator's own tables, lie behind tot.
struct TileTab {
    uint64_t ntiles;
    uint64_t *cnt, *base, *ibase, *bounds, *tot;
};
TileTab tile_tab(Workspace* ws, const char* scratch_name, uint64_t ntiles,
                 uint32_t bounds_words, size_t extra_bytes = 0);
// mat_scan over the table, then its totals on the host (a 16-byte copy into
// the named pinned buffer and ONE synchronisation of `st`): the outputs in
// all and the work items the write pass has to launch for the first out_cap.
struct MatFinish {
    uint64_t total, launch;
};
MatFinish mat_finish(Workspace* ws, const char* pinned_name, const TileTab& tab,
                     uint64_t out_cap, hipStream_t st);
// The count forms: the tile counts cnt[0..ntiles) (uint64_t or uint32_t)
// added to *total_dev, stream-ordered; traced when trace_name is not null.
template <class C>
void tile_total(Workspace* ws, const char* trace_name, const C* cnt, uint64_t ntiles,
                unsigned long long* total_dev, hipStream_t st);
// the bounds pass of an operator: one thread per tile, traced as `name`
template <class Kern, class... A>
inline void launch_tile_bounds(Workspace* ws, const char* name, Kern kern, uint64_t ntiles,
                               hipStream_t st, A... args) {
    TraceScope ts(ws, name, st);
    hipLaunchKernelGGL(kern, dim3((uint32_t)((ntiles + 255) / 256)), dim3(256), 0, st, args...);
    SMJ_CHECK(hipGetLastError());
}

// ---- bandjoin.hip : band join of sorted R and S (smj.h smj_dev_band_join)
// Every pair with s.key + lo <= r.key <= s.key + hi, S-major, as columns of
// the ABI's value_t / intkey_t (the key columns may be null); materialize()'s
// capacity and synchronisation rules.
uint64_t band_join(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                   int64_t lo, int64_t hi, void* r_out, void* s_out, void* r_key_out,
                   void* s_key_out, uint64_t out_cap, hipStream_t st);
// its count, added to *count_dev (stream-ordered, no synchronisation)
void band_join_count(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                     int64_t lo, int64_t hi, unsigned long long* count_dev, hipStream_t st);

// ---- asofjoin.hip : as-of join of sorted R and S (smj.h smj_dev_asof_join)
// Per S tuple one partner in R: the last at or before its key, the first at
// or after it, or the closer of the two (dir; the values of SMJ_ASOF_*),
// within `tolerance` and the key group of `group_shift` (0..63, 0: none).  Row
// i of every non-null column belongs to S[i]; the matched rows are added to
// *matched_dev unless it is null.  Stream-ordered, no synchronisation.
constexpr uint32_t kAsofBackward = 0, kAsofForward = 1, kAsofNearest = 2;
void asof_join(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
               uint32_t dir, bool strict, uint64_t tolerance, uint32_t group_shift,
               int64_t* r_index_out, void* r_payload_out, void* r_key_out,
               unsigned long long* matched_dev, hipStream_t st);

// ---- outerjoin.hip : outer join of sorted R and S (smj.h smj_dev_outer_join)
// The inner join's pairs in join_pairs' order and, in key order between them,
// the partnerless R tuples (keep & kOuterKeepR) and S tuples (keep &
// kOuterKeepS; the values of SMJ_OUTER_KEEP_*), as columns: positions in R
// and S (-1: absent), payloads and key as the ABI's value_t / intkey_t (0:
// absent); each may be null.  materialize()'s capacity rules; synchronises
// `st` once, not at all when nR or nS is 0.
constexpr uint32_t kOuterKeepR = 1, kOuterKeepS = 2;
uint64_t outer_join(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                    uint32_t keep, int64_t* r_index_out, int64_t* s_index_out,
                    void* r_payload_out, void* s_payload_out, void* key_out, uint64_t out_cap,
                    hipStream_t st);
// its number of rows, added to *count_dev (stream-ordered, no synchronisation)
void outer_join_count(Workspace* ws, const Tup* R, uint64_t nR, const Tup* S, uint64_t nS,
                      uint32_t keep, unsigned long long* count_dev, hipStream_t st);

// ---- groupagg.hip : grouped aggregation of a sorted relation (smj.h
// smj_dev_group_aggregate)
// One row per maximal run of equal key >> group_shift (0..63), in input
// order: the run's first key, its start and length, and the sum (int64,
// wrapping), minimum and maximum of its payloads, as columns of the ABI's
// intkey_t / int64 / value_t (each may be null).  Writes the first
// min(groups, out_cap) rows and returns the number of groups (synchronises
// `st` once; n == 0 returns 0 at once).
uint64_t group_aggregate(Workspace* ws, const Tup* in, uint64_t n, uint32_t group_shift,
                         void* key_out, int64_t* start_out, int64_t* count_out,
                         int64_t* sum_out, void* min_out, void* max_out, uint64_t out_cap,
                         hipStream_t st);
// its number of groups, added to *groups_dev (stream-ordered, no synchronisation)
void group_count(Workspace* ws, const Tup* in, uint64_t n, uint32_t group_shift,
                 unsigned long long* groups_dev, hipStream_t st);
uint32_t group_tile();  // elements of `in` a workgroup of its kernels handles

// ---- window.hip : window functions over a sorted relation (smj.h
// smj_dev_window)
// One row per tuple, PARTITION BY key >> group_shift (0..63) ORDER BY key,
// ROWS UNBOUNDED PRECEDING, by position in the input: the row of
// group_aggregate's table that holds the tuple, its position in its group, its
// rank and dense rank among the group's keys (both from 0), and the running
// sum (int64, wrapping), minimum and maximum of the payloads from the group's
// start to it, as columns of int64 / the ABI's value_t (each may be null).
// Every non-null column gets n rows.  Stream-ordered, no synchronisation;
// n == 0 or no column launches nothing.
void window(Workspace* ws, const Tup* in, uint64_t n, uint32_t group_shift, int64_t* group_out,
            int64_t* row_out, int64_t* rank_out, int64_t* dense_rank_out, int64_t* sum_out,
            void* min_out, void* max_out, hipStream_t st);
uint32_t window_tile();  // elements of `in` a workgroup of its kernels handles

// ---- frame.hip : sliding window frames over a sorted relation (smj.h
// smj_dev_window_frame)
// One row per tuple, window()'s groups, the frame ROWS (positions i + lo ..
// i + hi) or, with `range`, RANGE (keys key[i] + lo .. key[i] + hi, saturating)
// BETWEEN lo AND hi inside the tuple's group: where the frame starts (-1:
// empty), how many tuples it holds, the sum (int64, wrapping), minimum and
// maximum of their payloads and the payloads of its first and last tuple (0
// for an empty frame), as columns of int64 / the ABI's value_t (each may be
// null).  Every non-null column gets n rows.  Stream-ordered, no
// synchronisation; n == 0 or no column launches nothing.
void window_frame(Workspace* ws, const Tup* in, uint64_t n, uint32_t group_shift, bool range,
                  int64_t lo, int64_t hi, int64_t* start_out, int64_t* count_out,
                  int64_t* sum_out, void* min_out, void* max_out, void* first_out,
                  void* last_out, hipStream_t st);
uint32_t frame_tile();   // elements of `in` a workgroup of its tile kernels handles
uint32_t frame_block();  // the inner aligned block of its range minimum and maximum

// ---- datagen.hip
void gen_pk(Tup* out, uint64_t n, uint64_t first, uint64_t total,
            uint64_t seed, hipStream_t st);
void gen_fk(Tup* out, uint64_t n, uint64_t first, uint64_t total,
            uint64_t maxid, uint64_t seed, hipStream_t st);
void gen_zipf(Workspace* ws, Tup* out, uint64_t n, uint64_t first,
              uint64_t maxid, double theta, uint64_t seed, hipStream_t st);

}  // namespace smj
