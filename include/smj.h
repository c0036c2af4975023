/*
 * smj.h -- C ABI of the MI355X sort-merge-join library (libsmj_hip*.so).
 *
 * This header is the drop-in boundary for the m-way sort-merge-join hot path of
 * sdecoder/AVX-sort-merge-joins.  Every entry point below keeps the name,
 * argument meaning, pointer-swap conventions and data layout of the reference
 * function it replaces (cited as reference-path:line), so the reference's own
 * drivers (bench_sort, bench_partitioning, bench_multiwaymerge, tputbench,
 * sortmergejoins) and check_* tests compile against include/compat/ and link
 * against this library instead of the AVX objects.
 *
 * Tuple width is a compile-time choice, exactly like the reference
 * (configure --enable-key8B -> -DKEY_8B, src/types.h:23-29):
 *   default : 8-byte tuples  {int32 payload; int32 key}  -> libsmj_hip.so
 *   KEY_8B  : 16-byte tuples {int64 payload; int64 key}  -> libsmj_hip_k8.so
 *
 * Pointers handed to the reference-named functions may be host memory (the
 * library stages them through HBM and writes results back to the same host
 * addresses/layout) or device memory from hipMalloc (work stays in HBM, no
 * copies).  The smj_dev_* functions are the asynchronous device-resident form
 * used by bench.py: device pointers only, explicit HIP stream, no host sync.
 * Device pointers: aligned to 8 bytes for 8-byte tuples, to 16 bytes for
 * 16-byte tuples; nothing more is assumed.  Any tuple-granular slice of a
 * hipMalloc buffer is therefore a valid relation or output, used in place
 * (element columns -- value_t, intkey_t, int64 words -- to their element).
 *
 * Order of the sorted output (the parity contract):
 *   8-byte tuples : ascending signed-int64 order of the packed word
 *                   (key << 32 | (uint32)payload) == what the AVX path yields
 *                   for keys in the generators' domain (src/avxsort/avxcommon.h).
 *   16-byte tuples: ascending (key, payload), both signed int64 == the
 *                   reference scalar path (key-only std::sort,
 *                   src/scalarsort/scalarsort.c:41-50) with equal-key runs
 *                   canonicalised by payload.
 *
 * Errors: like the reference (no error codes), a HIP failure prints a message
 * and aborts; the library never falls back to a CPU implementation.
 */
#ifndef SMJ_H
#define SMJ_H

#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <inttypes.h>
#include <sys/time.h>
#include <pthread.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Data ABI (reference src/types.h:22-98). Layout is byte-identical, and the */
/* include guard is the reference's own (TYPES_H), so this header and the    */
/* reference's types.h can both be included in one translation unit.        */
/* ------------------------------------------------------------------------ */
#ifndef TYPES_H
#define TYPES_H
#ifdef KEY_8B
typedef int64_t intkey_t;   /* 16-byte tuples */
typedef int64_t value_t;
#else
typedef int32_t intkey_t;   /* 8-byte tuples (reference default) */
typedef int32_t value_t;
#endif

typedef struct tuple_t        tuple_t;
typedef struct relation_t     relation_t;
typedef struct result_t       result_t;
typedef struct threadresult_t threadresult_t;
typedef struct joinconfig_t   joinconfig_t;

/* payload first, then key: the reference packs an 8-byte tuple into one
 * little-endian word whose high half is the key (src/types.h:51-54). */
struct tuple_t {
    value_t  payload;
    intkey_t key;
};

struct relation_t {
    tuple_t * tuples;
    uint64_t  num_tuples;
};

struct threadresult_t {
    int64_t  nresults;
    void *   results;
    uint32_t threadid;
};

struct result_t {
    int64_t          totalresults;
    threadresult_t * resultlist;
    int              nthreads;
};

enum numa_strategy_t { RANDOM, RING, NEXT };

struct joinconfig_t {
    int NTHREADS;
    int PARTFANOUT;
    int SCALARSORT;
    int SCALARMERGE;
    int MWAYMERGEBUFFERSIZE;
    enum numa_strategy_t NUMASTRATEGY;
};
#endif /* TYPES_H */

/* ------------------------------------------------------------------------ */
/* Compile-time parameters (reference src/params.h:17-72, guard PARAMS_H_).  */
/* ------------------------------------------------------------------------ */
#ifndef PARAMS_H_
#define PARAMS_H_
#ifndef NRADIXBITS_DEFAULT
#define NRADIXBITS_DEFAULT 7
#endif
#ifndef PARTFANOUT_DEFAULT
#define PARTFANOUT_DEFAULT (1 << NRADIXBITS_DEFAULT)
#endif
#ifndef CACHE_LINE_SIZE
#define CACHE_LINE_SIZE 64
#endif
#ifndef L2_CACHE_SIZE
#define L2_CACHE_SIZE (256 * 1024)
#endif
#ifndef L3_CACHE_SIZE
#define L3_CACHE_SIZE (20 * 1024 * 1024)
#endif
/* one cache line of padding per partition (params.h:47) */
#ifndef CACHELINEPADDING
#define CACHELINEPADDING(FANOUT) ((FANOUT) * CACHE_LINE_SIZE / sizeof(tuple_t))
#endif
/* tail padding callers allocate behind R, S and temporaries (params.h:56) */
#ifndef RELATION_PADDING
#define RELATION_PADDING(NTHR, FANOUT) \
    ((NTHR) * CACHELINEPADDING(FANOUT) * sizeof(tuple_t))
#endif
#ifndef MWAY_MERGE_BUFFER_SIZE_DEFAULT
#define MWAY_MERGE_BUFFER_SIZE_DEFAULT L3_CACHE_SIZE
#endif
#define TUPLESPERCACHELINE (CACHE_LINE_SIZE / sizeof(tuple_t))
#define ALIGN_NUMTUPLES(N) \
    (((N) + TUPLESPERCACHELINE - 1) & ~(TUPLESPERCACHELINE - 1))
#endif /* PARAMS_H_ */

/* ------------------------------------------------------------------------ */
/* Radix partitioning (reference src/partition/partition.h:57-120).          */
/* Partition index of a tuple: ((key - 1) & (((1<<nbits)-1) << shift))      */
/*   >> shift (partition.c:29). Output is a stable scatter.                  */
/* ------------------------------------------------------------------------ */

/* partition.c:301-327 -- naive stable layout, partitions back to back. */
void partition_relation(relation_t ** partitions, relation_t * input,
                        relation_t * output, int radixbits, int shiftbits);

/* partition.c:329-354 -- stable scatter, every partition starts on a 64-byte
 * boundary (offsets advance by ALIGN_NUMTUPLES(count)). */
void partition_relation_optimized(relation_t ** partitions, relation_t * input,
                                  relation_t * output, uint32_t nbits,
                                  uint32_t shiftbits);

/* partition.c:356-385 -- same output as the optimized variant. */
void partition_relation_optimized_V2(relation_t ** partitions,
                                     relation_t * input, relation_t * output,
                                     uint32_t nbits, uint32_t shiftbits);

/* partition.c:422-436 -- histogram pass + plain copy (bandwidth probe). */
void histogram_memcpy_bench(relation_t ** partitions, relation_t * input,
                            relation_t * output, uint32_t nbits);

/* partition.h:38-43 (defined partition.c:93-149) -- the naive stable radix
 * cluster on bits [R, R + D) of key - 1 into outRel->tuples, partitions back
 * to back (no padding).  Like the reference it ADDS each partition's count to
 * hist[0 .. 2^D) and starts partition i at the prefix sum of the updated hist,
 * so the caller zeroes hist first for the usual layout. */
void radix_cluster(relation_t * outRel, relation_t * inRel, int32_t * hist,
                   int R, int D);

/* ------------------------------------------------------------------------ */
/* Sorting (reference src/avxsort/avxsort.h:35-57,                           */
/* src/avxsort/avxsort_multiway.h:35-55, src/scalarsort/scalarsort.h).       */
/* Result convention (avxsort.c:117-118,224-225): on return *outputptr       */
/* points at the sorted items, *inputptr at the other buffer; both buffers   */
/* may be clobbered.                                                         */
/* ------------------------------------------------------------------------ */
void avxsort_tuples(tuple_t ** inputptr, tuple_t ** outputptr, uint64_t nitems);
void avxsort_int64(int64_t ** inputptr, int64_t ** outputptr, uint64_t nitems);
/* avxsort.c:247-250 is an empty stub in the reference; here it sorts. */
void avxsort_int32(int32_t ** inputptr, int32_t ** outputptr, uint64_t nitems);
void avxsortmultiway_tuples(tuple_t ** inputptr, tuple_t ** outputptr,
                            uint64_t nitems);
void avxsortmultiway_int64(int64_t ** inputptr, int64_t ** outputptr,
                           uint64_t nitems);
/* scalarsort.c:41-50 sorts in place and swaps the pointers. */
void scalarsort_tuples(tuple_t ** inputptr, tuple_t ** outputptr,
                       uint64_t nitems);
void scalarsort_int64(int64_t ** inputptr, int64_t ** outputptr,
                      uint64_t nitems);
void scalarsort_int32(int32_t ** inputptr, int32_t ** outputptr,
                      uint64_t nitems);

/* The reference's in-register kernel inregister_sort_keyval32
 * (src/avxsort/avxsort_core.h:1213-1274, the compat header
 * include/compat/avxsort_core.h maps that name here), on nblocks consecutive
 * blocks of 16 int64 items: output row j of a block (items 4j..4j+3) is the
 * column {x[j], x[j+4], x[j+8], x[j+12]} after the reference's 4x4 odd-even
 * network of VMINPD/VMAXPD on the items as IEEE doubles, byte-identical to
 * the AVX kernel (NaNs and signed zeros included).  Runs on the device. */
void smj_inregister_sort_keyval32(const int64_t * items, int64_t * output,
                                  uint64_t nblocks);

/* ------------------------------------------------------------------------ */
/* Merging (reference src/merge/merge.h:35-97, avx_multiwaymerge.h:33-38,    */
/* scalar_multiwaymerge.h:31-78). Return value = tuples written.             */
/* ------------------------------------------------------------------------ */
uint64_t avx_merge_tuples(tuple_t * const inA, tuple_t * const inB,
                          tuple_t * const outp, const uint64_t lenA,
                          const uint64_t lenB);
uint64_t avx_merge_int64(int64_t * const inA, int64_t * const inB,
                         int64_t * const outp, const uint64_t lenA,
                         const uint64_t lenB);
uint64_t scalar_merge_tuples(tuple_t * const inA, tuple_t * const inB,
                             tuple_t * const outp, const uint64_t lenA,
                             const uint64_t lenB);
uint64_t scalar_merge_int64(int64_t * const inA, int64_t * const inB,
                            int64_t * const outp, const uint64_t lenA,
                            const uint64_t lenB);

/* avx_multiwaymerge.c:199-338. `fifobuffer`/`bufntuples` are accepted for
 * ABI compatibility; the GPU merge stages run heads in LDS instead of an
 * L3-resident FIFO tree. On return every parts[i] has been consumed:
 * parts[i]->tuples advanced by its count and parts[i]->num_tuples == 0,
 * as the reference leaves them (avx_multiwaymerge.c:268-272). */
uint64_t avx_multiway_merge(tuple_t * output, relation_t ** parts,
                            uint32_t nparts, tuple_t * fifobuffer,
                            uint32_t bufntuples);
uint64_t scalar_multiway_merge(tuple_t * output, relation_t ** parts,
                               uint32_t nparts, tuple_t * fifobuffer,
                               uint32_t bufntuples);
uint64_t scalar_multiway_merge_modulo(tuple_t * output, relation_t ** parts,
                                      uint32_t nparts, tuple_t * fifobuffer,
                                      uint32_t bufntuples);
uint64_t scalar_multiway_merge_bitand(tuple_t * output, relation_t ** parts,
                                      uint32_t nparts, tuple_t * fifobuffer,
                                      uint32_t bufntuples);

/* ------------------------------------------------------------------------ */
/* Joins (reference src/joins/joincommon.h:78-80,                            */
/* src/joins/sortmergejoin_multiway.h:37-38, sortmergejoin_mpsm.h).          */
/* ------------------------------------------------------------------------ */

/* Materialised join output (the reference's JOIN_MATERIALIZE build,
 * joincommon.c:256-289, sortmergejoin_multiway.c:565-598, main.c:609-626).
 * The reference takes chainedtuplebuffer_t and its functions from
 * tuple_buffer.h, which is not in its tree, so this is the library's own
 * definition of that interface: one growable host array holding one
 * <S.key, S.payload> tuple per match, in merge_join's R-major order (per key,
 * the S run repeated |R_k| times, keys ascending).  A pointer returned by
 * cb_next_writepos stays valid until the next write. */
#ifndef SMJ_TUPLE_BUFFER
#define SMJ_TUPLE_BUFFER
typedef struct chainedtuplebuffer_t {
    tuple_t * tuples;
    uint64_t  numtuples;
    uint64_t  capacity;
} chainedtuplebuffer_t;
chainedtuplebuffer_t * chainedtuplebuffer_init(void);
/* NULL is a no-op (main.c:621-626 frees every thread's list) */
void chainedtuplebuffer_free(chainedtuplebuffer_t * cb);
uint64_t chainedtuplebuffer_tuples(chainedtuplebuffer_t * cb);
tuple_t * cb_next_writepos(chainedtuplebuffer_t * cb);
#endif /* SMJ_TUPLE_BUFFER */

/* joincommon.c:239-312: number of (r, s) pairs with equal key between two
 * sorted runs, duplicates on both sides included.  A non-NULL `output` is a
 * chainedtuplebuffer_t that receives the matches appended (JOIN_MATERIALIZE);
 * they are produced on the device (smj_dev_materialize) and copied back. */
uint64_t merge_join(tuple_t * rtuples, tuple_t * stuples, const uint64_t numR,
                    const uint64_t numS, void * output);

/* Materialisation switch of the join entry points (the reference decides it
 * at compile time with -DJOIN_MATERIALIZE; the library cannot see the
 * caller's flags): on, sortmergejoin_multiway / _multipass / _mpsm hand the
 * whole output in result->resultlist[0].results as a chainedtuplebuffer_t
 * (the other threads' lists stay NULL; m-pass fills one list per thread, as
 * its threads own disjoint partitions).  Default: the environment variable
 * SMJ_MATERIALIZE (unset = off).  The switch is process-wide, like the
 * compile-time flag it stands for: every reference-named join in the
 * process sees the last value set (an atomic).  Callers that need a mode per
 * call use smj_join below instead. */
void smj_set_materialize(int on);

/* The reference's three join algorithms with the materialisation chosen per
 * call (library extension; the reference fixes it per build): algo 0 =
 * sortmergejoin_multiway, 1 = sortmergejoin_multipass, 2 =
 * sortmergejoin_mpsm; materialize 1 / 0 overrides the process switch for this
 * call only, -1 follows it.  Returns what the named function returns (NULL
 * for an unknown algo). */
result_t * smj_join(relation_t * relR, relation_t * relS, joinconfig_t * joincfg,
                    int algo, int materialize);

/* main.c:609-614 (PERSIST_RELATIONS + JOIN_MATERIALIZE): append the
 * materialised result to `filename` in the text format of write_relation
 * (src/datagen/generator.c:200-213): a "#KEY, VAL" line, then "key payload"
 * per tuple, both printed with %d as the reference does (for 16-byte tuples
 * that is the low 32 bits of each field, what its int64 arguments print as
 * on x86-64).  The reference calls this function but never defines it. */
void write_result_relation(result_t * result, const char * filename);

/* joincommon.c:214-227: the drivers' timing line ("NUM-TUPLES = ...
 * TOTAL-TIME-USECS = ... TUPLES-PER-SECOND = ..."), host-side.  Declared in
 * the reference only by joincommon.h (some drivers define their own
 * print_timing), so the compat headers other than joincommon.h hide it. */
#ifndef SMJ_COMPAT_HIDE_PRINT_TIMING
void print_timing(uint64_t numtuples, struct timeval * start,
                  struct timeval * end, FILE * out);
#endif

/* joincommon.h:99-100 (defined joincommon.c:397-500): 1 when the keys of
 * the `nitems` tuples at `items` (a tuple_t array passed as int64_t*) never
 * decrease, starting from key 0, else 0.  Without KEY_8B it prints the
 * reference's "[WARN ] Equal items" line at the first repeated key before any
 * decrease and its "[ERROR]" line at the first decrease; with KEY_8B it
 * prints nothing.  The scan runs on the device. */
int is_sorted_helper(int64_t * items, uint64_t nitems);

/* joincommon.h:101-103 (defined joincommon.c:503-515): prints whether R and
 * S are sorted ("%d-thread -> R is sorted, size = %d"). */
void check_sorted(int64_t * R, int64_t * S, uint64_t nR, uint64_t nS, int my_tid);

/* joincommon.c (not in joincommon.h's prose): merge_join with an
 * interpolation search for the start; same count as merge_join. */
uint64_t merge_join_interpolation(tuple_t * rtuples, tuple_t * stuples,
                                  const uint64_t numR, const uint64_t numS,
                                  void * output);

/* The thread scaffolding of the reference joins (joincommon.h:40-44,
 * 105-155), layout-identical so that drivers with their own join thread
 * (tputbench.c:124-144) run unchanged on sortmergejoin_initrun below. */
#ifndef SMJ_ARG_T
#define SMJ_ARG_T
typedef struct arg_t arg_t;
typedef struct relationpair_t relationpair_t;
struct arg_t {
    tuple_t *  relR;
    tuple_t *  relS;
    tuple_t *  tmp_partR;   /* partitioning output, per thread */
    tuple_t *  tmp_partS;
    tuple_t *  tmp_sortR;   /* sorting output, per thread */
    tuple_t *  tmp_sortS;
    int32_t numR;
    int32_t numS;
    int32_t my_tid;
    int     nthreads;
    joinconfig_t * joincfg;
    pthread_barrier_t * barrier;
    int64_t result;
    relationpair_t ** threadrelchunks;
    tuple_t ** sharedmergebuffer;
    uint32_t ** histR;      /* mpsm-specific */
    tuple_t * tmpRglobal;
    uint64_t totalR;
#ifdef JOIN_MATERIALIZE
    threadresult_t * threadresult;
#endif
    struct timeval start, end;
    uint64_t part, sort, mergedelta, merge, join;
} __attribute__((aligned(CACHE_LINE_SIZE)));
struct relationpair_t {
    relation_t R;
    relation_t S;
};
#endif /* SMJ_ARG_T */

/* joincommon.c:29-212: allocates the per-thread temporaries (partition and
 * sort outputs, RELATION_PADDING behind each), slices R and S into T
 * contiguous chunks, runs `jointhread` on T pthreads sharing one barrier,
 * sums args[i].result into a malloc'd result_t and prints the stats lines
 * from args[0]'s timers.  The join thread's own calls (partition, sort,
 * merge, merge_join) are this library's device entry points.  Host-side
 * orchestration only: no tuple is touched here. */
result_t * sortmergejoin_initrun(relation_t * relR, relation_t * relS,
                                 joinconfig_t * joincfg,
                                 void * (*jointhread)(void *));

/* sortmergejoin_multiway.c:50-61: m-way sort-merge join. Returns a malloc'd
 * result_t (caller frees resultlist and the struct, main.c:629-632) whose
 * totalresults is the match count; NULL for a non-power-of-2 NTHREADS as the
 * reference does. NTHREADS only selects the reference-visible partition
 * fan-out checks: the whole join runs on the current HIP device. */
result_t * sortmergejoin_multiway(relation_t * relR, relation_t * relS,
                                  joinconfig_t * joincfg);

/* sortmergejoin_multipass.c:51-736 (m-pass): sort R and S completely, then
 * one merge-join scan; same result contract as sortmergejoin_multiway. */
result_t * sortmergejoin_multipass(relation_t * relR, relation_t * relS,
                                   joinconfig_t * joincfg);

/* sortmergejoin_mpsm.c:38-45 is a stub that exits in the reference; SURVEY.md
 * §2 row 9 and BASELINE configs[4] make it the multi-GPU join, and here it is
 * that: G = min(NTHREADS, visible GPUs) ranks in this process, one host thread
 * and one GPU each (the reference's T threads, joincommon.c:118-165, on
 * contiguous chunks of R and S, :127-139).  Every rank range-partitions its
 * chunks on its GPU, the partitions go to their owner GPUs over RCCL (grouped
 * ncclSend/ncclRecv, peers in NEXT order, numa_shuffle.c:83; the co-partition
 * exchange of sortmergejoin_multiway.c:463-556), each GPU sorts and joins the
 * contiguous key range it owns, and the counts are all-reduced
 * (ncclAllReduce).  totalresults = the global count; resultlist[g].nresults
 * = rank g's; with materialisation resultlist[g].results holds rank g's
 * matches (ranks in key order).  Keys are planned as 1..|R| like the m-way
 * join and verified (a key outside -> the measured range). */
result_t * sortmergejoin_mpsm(relation_t * relR, relation_t * relS,
                              joinconfig_t * joincfg);

/* The multi-GPU join of sortmergejoin_mpsm with its outputs (library
 * extension).  nranks ranks (0 = one per visible GPU); R and S in host memory
 * or in device memory any rank's GPU can read; rank g takes the g-th chunk of
 * each (the last one the rest).  key_min <= key_max: the key range (keys
 * outside it are legal but unbalance the ranks); otherwise 1..nR, verified.
 * sortedR / sortedS (optional, nR / nS tuples, host or device): the sorted
 * relations, the ranks' shares concatenated in rank order -- each rank owns
 * one contiguous key range, so this is the globally sorted relation.
 * rank_counts (optional, 2 * nranks): the tuples of R and of S each rank
 * sorted.  Returns the number of matching pairs.  Device inputs are read on
 * the ranks' own streams with no ordering against any caller stream: the
 * caller finishes every write to R and S before the call. */
#define SMJ_MG_COPY     1u  /* collectives by device copies instead of RCCL:
                               ranks may share a GPU (rank g on device g mod
                               the visible count); every exchange synchronises */
#define SMJ_MG_NOPLANES 2u  /* no 48-bit planes: 64-bit words or tuples */
#define SMJ_MG_ONECALL  4u  /* the local join in one call (not staged) */
#define SMJ_MG_SAMPLED  8u  /* sampled exchange partitions (default: one rank) */
#define SMJ_MG_EXACT   16u  /* exact exchange partitions (default: > 1 rank) */
typedef struct smj_mgpu_stats {
    int      layout;      /* of the exchange: 0 tuples, 1 64-bit words, 2 48-bit planes */
    uint32_t pbits;       /* exchange partitions = 2^pbits */
    int      attempts;    /* exchange attempts of rank 0 (2 = none repeated) */
    int      replans;     /* the guessed key range replaced by the measured one */
    uint64_t sent_bytes;  /* rows rank 0 sent to other ranks */
    uint64_t recv_bytes;  /* ... and received */
    int64_t  key_min;     /* the global plan's range */
    int64_t  key_max;
    double   ms;          /* host wall time of the call */
    /* device phases of the call on the rank's streams (HIP events), ms.  The
     * first five are consecutive on the rank's main stream and add up to
     * busy_ms: the range partitions of R and S (every attempt); their table
     * messages (k_xsend, the table exchange, k_xrecv, the summary copy); the
     * main stream waiting (host decisions and the row exchange the local work
     * did not hide); the local join (tile pass, group pass and count, both
     * stages); the count's all-reduce.  rows_ms: the row exchange on the
     * rank's row stream, which overlaps them. */
    double   partition_ms;
    double   tables_ms;
    double   wait_ms;
    double   join_ms;
    double   reduce_ms;
    double   busy_ms;
    double   rows_ms;
} smj_mgpu_stats;
int64_t smj_mgpu_join(const tuple_t * R, uint64_t nR, const tuple_t * S, uint64_t nS,
                      int nranks, uint32_t flags, int64_t key_min, int64_t key_max,
                      tuple_t * sortedR, tuple_t * sortedS, uint64_t * rank_counts,
                      smj_mgpu_stats * stats);
/* The multi-GPU join over ranks whose slices already lie on their GPUs (the
 * layout of a relation sharded over the node's HBM): rank g reads R[g]
 * (nR[g] tuples) and S[g] (nS[g]), host memory or device memory of GPU g, and
 * runs on GPU g (SMJ_MG_COPY: g mod the visible count).  Otherwise as
 * smj_mgpu_join; the sorted shares stay on the ranks' GPUs
 * (smj_mgpu_last_sorted).  key_min <= key_max: the global key range;
 * otherwise keys 1..sum(nR), verified. */
int64_t smj_mgpu_join_slices(const tuple_t * const * R, const uint64_t * nR,
                             const tuple_t * const * S, const uint64_t * nS, int nranks,
                             uint32_t flags, int64_t key_min, int64_t key_max,
                             uint64_t * rank_counts, smj_mgpu_stats * stats);
/* Rank `rank`'s statistics of the last smj_mgpu_join / _slices call (its
 * phases; `ms` is the call's host time).  Returns 0, or -1 when there is no
 * such rank. */
int smj_mgpu_last_stats(int rank, smj_mgpu_stats * out);
/* Device pointers to rank `rank`'s sorted shares of the last smj_mgpu_join /
 * _slices call (on the rank's GPU, valid until the next call) and their
 * sizes.  Returns 0, or -1 when there is no such rank. */
int smj_mgpu_last_sorted(int rank, tuple_t ** sortedR, uint64_t * nR, tuple_t ** sortedS,
                         uint64_t * nS);
/* Rank `rank`'s workspace in the in-process group of the last smj_mgpu_join
 * / _slices call (its kernel trace: smj_trace_*), NULL when there is none. */
struct smj_workspace * smj_mgpu_group_workspace(int rank);
/* Frees the ranks' devices buffers, streams and communicators (kept across
 * calls of one configuration). */
void smj_mgpu_release(void);

/* The same join with one rank per PROCESS (one process per GPU, e.g. under
 * torch.distributed.run): rank 0 gets an id (smj_mgpu_unique_id: writes up to
 * `cap` bytes, returns their count, 128), every process passes it to
 * smj_mgpu_comm_init on its current device, then every rank calls
 * smj_mgpu_rank_join with its own slices of R and S (host, or device memory
 * of its GPU).  key_min <= key_max: the global key range, the same on every
 * rank; otherwise keys 1..guess_max (the global |R|), verified.  *sortedR /
 * *sortedS receive device pointers to the rank's sorted share (*nR_out /
 * *nS_out tuples, one contiguous key range, ranks in order), valid until the
 * next call on the communicator.  Returns the global match count on every
 * rank.  flags: SMJ_MG_NOPLANES / _ONECALL / _SAMPLED / _EXACT. */
typedef struct smj_mgpu_comm smj_mgpu_comm;
int smj_mgpu_unique_id(void * out, int cap);
smj_mgpu_comm * smj_mgpu_comm_init(const void * id, int nranks, int rank);
int64_t smj_mgpu_rank_join(smj_mgpu_comm * comm, const tuple_t * R, uint64_t nR,
                           const tuple_t * S, uint64_t nS, uint32_t flags,
                           int64_t key_min, int64_t key_max, uint64_t guess_max,
                           tuple_t ** sortedR, uint64_t * nR_out, tuple_t ** sortedS,
                           uint64_t * nS_out, smj_mgpu_stats * stats);
/* copies the rank's sorted shares of the last smj_mgpu_rank_join (host or
 * device destinations; NULL skips one) */
void smj_mgpu_rank_sorted(smj_mgpu_comm * comm, tuple_t * outR, tuple_t * outS);
/* the rank's workspace (its kernel trace: smj_trace_*) */
struct smj_workspace * smj_mgpu_comm_workspace(smj_mgpu_comm * comm);
void smj_mgpu_comm_destroy(smj_mgpu_comm * comm);

/* ------------------------------------------------------------------------ */
/* Device-resident asynchronous API (no reference counterpart: this is the   */
/* form a GPU-aware caller binds).  All pointers are device pointers,        */
/* `stream` is a hipStream_t (NULL = default stream).                        */
/* ------------------------------------------------------------------------ */
typedef void * smj_stream_t;

/* Tuple width this library was built for (8 or 16). */
int smj_tuple_bytes(void);
/* Name of the device the library initialised, for logs. */
const char * smj_device_name(void);

/* Opaque reusable scratch (device memory).  One per stream/thread: calls on
 * one workspace must be ordered on one stream (they share its scratch and
 * the group pass's argument slot). */
typedef struct smj_workspace smj_workspace;
smj_workspace * smj_workspace_create(void);
void smj_workspace_destroy(smj_workspace * ws);

/* Layouts the sorts and joins on `ws` may not use (NULL: the calling thread's
 * workspace behind the reference-named entry points).  Default 0: every
 * layout allowed, each taken where it applies; the results
 * are the same whichever layout runs.  For A/B measurements and tests. */
#define SMJ_LAYOUT_NO_P48      1u  /* no 48-bit words in two planes */
#define SMJ_LAYOUT_NO_PACKED   2u  /* no 64-bit packed words (16-byte tuples) */
#define SMJ_LAYOUT_NO_SAMPLED  4u  /* exact histogram + scatter level-1 partition */
#define SMJ_LAYOUT_SAMPLE_PLAN 8u  /* without a key-range hint: plan from a device
                                      sample instead of from the relation size */
#define SMJ_LAYOUT_NO_P32     16u  /* no 32-bit words (tiny payloads) */
#define SMJ_LAYOUT_NO_P96     32u  /* no 12-byte elements (payloads no packed word
                                      holds: 16-byte tuples instead) */
void smj_workspace_set_layouts(smj_workspace * ws, uint32_t off);
/* The intermediate layout the last device sort or join on `ws` (NULL: the
 * calling thread's workspace) finished in: tuples, 64-bit packed words,
 * 48-bit words in two planes, 32-bit words, 12-byte elements (the full
 * payload and a 32-bit key offset, in two planes); -1 before the first
 * call. */
#define SMJ_LAYOUT_USED_TUPLES 0
#define SMJ_LAYOUT_USED_WORDS  1
#define SMJ_LAYOUT_USED_P48    2
#define SMJ_LAYOUT_USED_P32    3
#define SMJ_LAYOUT_USED_P96    4
int smj_workspace_last_layout(smj_workspace * ws);
/* The stable partition (smj_dev_partition, partition_relation*, radix_cluster)
 * ranks with lane-ordered LDS atomics where the device passes
 * smj_selfcheck_lds_order, and with wave ballots where it does not.  on != 0:
 * the stable partitions on `ws` (NULL: the calling thread's workspace) choose
 * their scatter kernel as if the device had failed that check; 0 (default):
 * as the device answers.  The results are the same.  For tests. */
void smj_workspace_force_ballot_ranks(smj_workspace * ws, int on);
/* The scatter kernels the last stable partition on `ws` (NULL: the calling
 * thread's workspace) launched, as a mask: one of the four kernels (DESIGN.md
 * §3), twice over with SMJ_SCATTER_TWO_PASS for a digit wider than 12 bits;
 * 0 before the first call, and no kernel's bit for a partition of no tuples.
 * Set on the host where the launch is decided: no copy and no synchronisation
 * is added.  For tests. */
#define SMJ_SCATTER_ATOMIC         1u  /* k_scatter_swp: LDS-atomic ranks */
#define SMJ_SCATTER_BALLOT_WC      2u  /* k_scatter_swc: ballot ranks, write combining */
#define SMJ_SCATTER_BALLOT_512X16  4u  /* k_scatter on 512 x 16 tiles */
#define SMJ_SCATTER_BALLOT_256X8   8u  /* k_scatter on 256 x 8 tiles */
#define SMJ_SCATTER_TWO_PASS      16u  /* two stable passes and a padding copy */
uint32_t smj_workspace_last_scatter(smj_workspace * ws);
/* What became of the groups that the group pass could not finish in LDS and
 * queued for the skew path, in the last bucket pass (the tile and group passes
 * of a device sort or join) that completed on `ws` (NULL: the calling
 * thread's workspace).  An attempt that is repeated in another layout or with
 * another plan (region overflow, payloads that do not pack, a key outside a
 * guessed range) leaves the record as it was.  Host values the pass holds
 * anyway: no copy and no synchronisation is added for them.  For tests.
 * Returns 0, or -1 (and leaves *out) before the first such pass. */
typedef struct smj_skew_stats {
    uint32_t tpl;        /* tile runs a lane of the last group pass took: 2 or 4 */
    uint32_t queued;     /* groups in the queue (0: the skew path did not run) */
    uint32_t empty;      /* ... with no tuple in either relation */
    uint32_t small;      /* ... taken by one workgroup each */
    uint32_t large;      /* ... taken by the split kernels */
    uint32_t items;      /* work items of the large ones */
    uint32_t inexact;    /* ... whose digits did not order the keys (every one
                            when the plan has key bits below the last digit) */
    uint32_t unordered;  /* ... with equal keys out of payload order */
    uint32_t resorted;   /* groups handed to the segmented merge sort */
    uint32_t recounted;  /* pairs handed to the batched merge-join count */
} smj_skew_stats;
int smj_workspace_skew_stats(smj_workspace * ws, smj_skew_stats * out);
/* What the last k-way merge (smj_dev_multiway_merge_host, avx_multiway_merge
 * and whatever else merges k runs) on `ws` (NULL: the calling thread's
 * workspace) did.  form, k and D are host values, stored where the merge
 * chooses its form.  queued is word 0 of the merge's overflow queue on the
 * device, read here with one blocking copy: the caller must have synchronised
 * the merge's stream before the call, and this accessor is the only place a
 * copy is added -- none to the merge itself.  For tests.  Returns 0, or -1
 * (and leaves *out) before the first k-way merge on the workspace. */
#define SMJ_MERGE_NONE    0u  /* no tuples: nothing launched */
#define SMJ_MERGE_BUCKETS 1u  /* 3..256 runs: one pass over 2^D value buckets */
#define SMJ_MERGE_TREE    2u  /* 1, 2 or more than 256 runs: 2-way merge passes */
typedef struct smj_merge_stats {
    uint32_t form;    /* SMJ_MERGE_* */
    uint32_t k;       /* runs, empty ones included */
    uint32_t D;       /* SMJ_MERGE_BUCKETS: bucket bits, else 0 */
    uint32_t queued;  /* SMJ_MERGE_BUCKETS: buckets larger than the LDS buffer,
                         merged by the overflow kernel; else 0 */
} smj_merge_stats;
int smj_workspace_merge_stats(smj_workspace * ws, smj_merge_stats * out);
/* Workgroups of the tile-pass kernel that intermediate layout `layout`
 * (SMJ_LAYOUT_USED_P48 or _P32) takes which the runtime places on one compute
 * unit (hipOccupancyMaxActiveBlocksPerMultiprocessor) at the dynamic LDS size
 * of a launch with 2^d2_bits level-2 digits.  The 48-bit planes are staged in
 * turn so that two 16384-element tiles share a compute unit:
 * this is the guard against losing the second one to a register or LDS
 * budget.  -1 for a layout without such a kernel or d2_bits beyond the
 * plan's limit. */
int smj_tilepass_occupancy(int layout, uint32_t d2_bits);

/* Stable radix partition, the device form of partition_relation*.
 * padded != 0 -> partition_relation_optimized layout.
 * hist_out / off_out (device, int64[1<<nbits]) receive per-partition counts
 * and start offsets in tuples. */
void smj_dev_partition(smj_workspace * ws, const tuple_t * in, uint64_t n,
                       tuple_t * out, uint32_t nbits, uint32_t shiftbits,
                       int padded, int64_t * hist_out, int64_t * off_out,
                       smj_stream_t stream);

/* Full sort of n tuples into `out`.  `out` may equal or overlap `in`: the
 * sort then runs into workspace scratch and is copied over the input at the
 * end (one more pass over n tuples); otherwise `in` is left untouched. */
void smj_dev_sort(smj_workspace * ws, const tuple_t * in, uint64_t n,
                  tuple_t * out, smj_stream_t stream);

/* Merge two sorted runs.  The call takes no workspace: its tile table lies in
 * the calling thread's workspace, whatever `stream` is, so like `ws`
 * elsewhere it serves one stream at a time -- two streams of one thread would
 * share that table. */
void smj_dev_merge2(const tuple_t * a, uint64_t na, const tuple_t * b,
                    uint64_t nb, tuple_t * out, smj_stream_t stream);

/* k-way merge of sorted device runs whose pointers/lengths are host arrays.
 * Stream-ordered: for 3..256 runs no host synchronisation (round 5; the
 * host arrays may be reused as soon as the call returns). */
void smj_dev_multiway_merge_host(smj_workspace * ws,
                                 const tuple_t * const * runs,
                                 const uint64_t * lens, uint32_t k,
                                 tuple_t * out, smj_stream_t stream);

/* Merge-join count of two sorted runs; result is ADDED to *count_dev. */
void smj_dev_merge_join_count(const tuple_t * r, uint64_t nr,
                              const tuple_t * s, uint64_t ns,
                              unsigned long long * count_dev,
                              smj_stream_t stream);

/* Materialised merge join of two sorted relations: the output of
 * merge_join built with JOIN_MATERIALIZE (src/joins/joincommon.c:256-289),
 * one <S.key, S.payload> tuple per match, R-major -- per key, the S run
 * repeated |R_k| times, keys ascending -- as one flat array (the reference's
 * chained buffer, tuple_buffer.h, is not in its tree).  Writes the first
 * min(total, out_cap) tuples to `out` (device) and returns the total number
 * of matches; out_cap = 0 only counts.  Synchronises `stream` once. */
uint64_t smj_dev_materialize(smj_workspace * ws, const tuple_t * sortedR,
                             uint64_t nR, const tuple_t * sortedS, uint64_t nS,
                             tuple_t * out, uint64_t out_cap, smj_stream_t stream);

/* The join index of two sorted relations: which rows matched.  For output
 * position q, in exactly the order smj_dev_materialize emits -- keys
 * ascending; per key R-major: for each R tuple of the key's run in sorted
 * order, the whole S run in sorted order -- r_payload_out[q] is the payload
 * of the matching R tuple, s_payload_out[q] that of the matching S tuple
 * (the payload column of smj_dev_materialize's output), and key_out[q] the
 * key, unless key_out is NULL.  With row ids as payloads these are the
 * columns a caller gathers its other columns with.  Three separate device
 * columns of out_cap elements each: the first min(total, out_cap) positions
 * are written, the rest are left alone, and the total number of matches is
 * returned (it may exceed 2^32); out_cap = 0 only counts.  Synchronises
 * `stream` once. */
uint64_t smj_dev_join_pairs(smj_workspace * ws, const tuple_t * sortedR, uint64_t nR,
                            const tuple_t * sortedS, uint64_t nS, value_t * r_payload_out,
                            value_t * s_payload_out, intkey_t * key_out /* may be NULL */,
                            uint64_t out_cap, smj_stream_t stream);

/* Semi join (anti = 0): the tuples of sortedS whose key occurs in sortedR,
 * in sorted order; anti join (anti != 0): those whose key does not.  The
 * same filter on the R side is the call with the relations swapped.  Writes
 * the first min(total, out_cap) tuples to `out` (device) and returns the
 * total; out_cap = 0 only counts.  nR = 0 gives nothing (semi) or all of S
 * (anti).  Synchronises `stream` once (not at all when nR or nS is 0). */
uint64_t smj_dev_semi_join(smj_workspace * ws, const tuple_t * sortedR, uint64_t nR,
                           const tuple_t * sortedS, uint64_t nS, tuple_t * out,
                           uint64_t out_cap, int anti, smj_stream_t stream);

/* Band join of two sorted relations: every pair (r, s) with
 * s.key + lo <= r.key <= s.key + hi (the library's own; the join a sort-merge
 * library offers and a hash join cannot).
 * Predicate: evaluated without wrap-around.  The 8-byte library computes
 *   s.key + lo and s.key + hi in int64, so a lo or hi beyond the int32 range
 *   means "unbounded on that side"; the 16-byte library saturates the sums at
 *   INT64_MIN and INT64_MAX.  An S tuple whose whole band lies outside int64
 *   (s.key + lo > INT64_MAX or s.key + hi < INT64_MIN) has no partner.
 * Empty calls: lo > hi, nR == 0 or nS == 0 return 0, launch nothing and do
 *   not synchronise.
 * Order: S-major, by position in the sorted arrays -- for each S tuple in
 *   sorted order, its partners sortedR[lb .. ub) in sorted order.  This is
 *   deterministic given the sorted inputs (8-byte tie order included).  It is
 *   NOT smj_dev_join_pairs' order for lo = hi = 0 when a key repeats on both
 *   sides (that one is R-major per key); the two coincide when, for every
 *   key, one side holds it at most once.
 * Output: position q gets the payloads of its R and S tuple in
 *   r_payload_out[q] and s_payload_out[q] and their keys in r_key_out[q] and
 *   s_key_out[q] (each key column may be NULL).  The first
 *   min(total, out_cap) positions of every non-NULL column are written, the
 *   rest are left alone, and the total is returned (it may exceed 2^32);
 *   out_cap = 0 only counts, and the payload columns may then be NULL.
 *   Synchronises `stream` once. */
uint64_t smj_dev_band_join(smj_workspace * ws, const tuple_t * sortedR, uint64_t nR,
                           const tuple_t * sortedS, uint64_t nS, int64_t lo, int64_t hi,
                           value_t * r_payload_out, value_t * s_payload_out,
                           intkey_t * r_key_out /* may be NULL */,
                           intkey_t * s_key_out /* may be NULL */,
                           uint64_t out_cap, smj_stream_t stream);

/* Its count only, ADDED to *count_dev (device), stream-ordered like
 * smj_dev_merge_join_count: no host synchronisation (the workspace's tables
 * grow on a first call).  The same predicate and empty calls. */
void smj_dev_band_join_count(smj_workspace * ws, const tuple_t * sortedR, uint64_t nR,
                             const tuple_t * sortedS, uint64_t nS, int64_t lo, int64_t hi,
                             unsigned long long * count_dev, smj_stream_t stream);

/* As-of join of two sorted relations: for every S tuple ONE partner in R, the
 * nearest R tuple at or before its key, at or after it, or on either side
 * ("the quote in force at each trade", merge_asof, ASOF JOIN; the library's
 * own, and like the band join one that only a sort-based library offers).
 * mode: one of the directions below, optionally or-ed with SMJ_ASOF_STRICT;
 *   any other value aborts with a message. */
#define SMJ_ASOF_BACKWARD 0u  /* B: the last position p with sortedR[p].key <= s.key  */
#define SMJ_ASOF_FORWARD  1u  /* F: the first position p with sortedR[p].key >= s.key */
#define SMJ_ASOF_NEAREST  2u  /* B or F, the smaller |s.key - r.key|; equal: B        */
#define SMJ_ASOF_STRICT   4u  /* or-ed in: equal keys are no partners (< and >)       */
/* Candidates: taken by position in the sorted arrays, so the result is
 *   deterministic given the sorted inputs (8-byte tie order included): among
 *   R tuples with equal keys backward takes the last and forward the first.
 *   With SMJ_ASOF_STRICT B is the last position with a key < s.key and F the
 *   first with a key > s.key.
 * tolerance: a candidate counts only if |s.key - r.key| <= tolerance, the
 *   distance taken as an unsigned 64-bit value without wrap-around (the
 *   difference of two int64 keys fits; the 8-byte library widens its int32
 *   keys first).  UINT64_MAX: no limit.
 * group_shift: 0 for no groups; for 1..63 a candidate counts only if
 *   (r.key >> group_shift) == (s.key >> group_shift), an arithmetic shift of
 *   the key widened to int64 -- the `by` of an as-of join for keys built as
 *   group << t | time.  The shift is monotone, so a group is one contiguous
 *   range of sortedR and the filter on the two candidates is exact: if B lies
 *   in a lower group, no R tuple of the S tuple's group is at or before it.
 *   Values above 63 abort with a message.
 * SMJ_ASOF_NEAREST: B and F are each filtered on their own by tolerance and
 *   group; of the survivors the one at the smaller distance wins, B on equal
 *   distances.
 * Output: row i belongs to sortedS[i], and every non-NULL column gets all nS
 *   rows: a matched row the partner's position in sortedR (r_index_out), its
 *   payload and its key; an unmatched row -1 in r_index_out and 0 in the other
 *   two.  Nothing is written beyond row nS - 1.  The number of matched rows
 *   is ADDED to *matched_dev (device), like smj_dev_band_join_count's count,
 *   unless it is NULL.  All three columns NULL with matched_dev non-NULL is
 *   the count form; everything NULL launches nothing.
 * Empty calls: nS == 0 launches nothing; nR == 0 writes every row as
 *   unmatched and adds 0.
 * Order: stream-ordered, no host synchronisation (the workspace's tables
 *   grow on a first call).  The inputs are left untouched; the outputs must
 *   not overlap them.  Alignment as for the rest of the device API:
 *   tuple-granular slices of a hipMalloc buffer, columns aligned to their
 *   element. */
void smj_dev_asof_join(smj_workspace * ws, const tuple_t * sortedR, uint64_t nR,
                       const tuple_t * sortedS, uint64_t nS, uint32_t mode,
                       uint64_t tolerance, uint32_t group_shift,
                       int64_t * r_index_out /* may be NULL */,
                       value_t * r_payload_out /* may be NULL */,
                       intkey_t * r_key_out /* may be NULL */,
                       unsigned long long * matched_dev /* may be NULL */,
                       smj_stream_t stream);

/* Outer join of two sorted relations (non-decreasing keys): the inner join's
 * pairs and, in key order between them, the tuples without a partner, the
 * missing side NULL -- one merge, and an output that is still sorted by key
 * (the library's own; a hash join gives no such order).  NULL is what the
 * as-of join writes for an unmatched row: -1 in an index column, 0 in a value
 * column.
 * keep: 0 is the inner join, SMJ_OUTER_KEEP_R the left outer join with R
 *   preserved, SMJ_OUTER_KEEP_S the left outer join with S preserved, both
 *   together the full outer join; any other bit aborts with a message. */
#define SMJ_OUTER_KEEP_R 1u   /* R tuples without a partner are kept (s side null) */
#define SMJ_OUTER_KEEP_S 2u   /* S tuples without a partner are kept (r side null) */
/* Everything below is defined by position in the sorted arrays, so the result
 *   is deterministic given the inputs (8-byte tie order included).
 * Order: rows come in ascending order of the union of the keys of R and S, as
 *   signed keys.  For a key present on both sides the rows are R-major,
 *   exactly smj_dev_join_pairs' order for that key: for each R tuple of the
 *   run in sorted order, the whole S run in sorted order.  For a key only in
 *   R, with SMJ_OUTER_KEEP_R, the rows are the R run in sorted order, one row
 *   each; without it there are none.  A key only in S likewise with
 *   SMJ_OUTER_KEEP_S.  With keep == 0 the rows are smj_dev_join_pairs' rows,
 *   position for position.
 * Columns: row q has the positions of its tuples in sortedR and sortedS in
 *   r_index_out[q] and s_index_out[q] (an absent side: -1), their payloads in
 *   r_payload_out[q] and s_payload_out[q] (an absent side: 0), and its key in
 *   key_out[q], taken from whichever side is present.  Any subset of the five
 *   columns may be NULL.
 * Capacity: the first min(total, out_cap) rows of every non-NULL column are
 *   written, everything else is left alone, and the total is returned (it may
 *   exceed 2^32).  out_cap = 0, or all columns NULL, only counts.
 *   Synchronises `stream` at most once.
 * Empty calls: nR == 0 && nS == 0 returns 0, launches nothing and does not
 *   synchronise.  With one side empty the result is 0 rows, or the other
 *   relation row for row with the empty side null, according to keep (and no
 *   synchronisation).
 * Buffers: the inputs are left untouched; the outputs must not overlap them.
 *   Alignment as for the rest of the device API: tuple-granular slices of a
 *   hipMalloc buffer (for the 8-byte library also one at an address that is
 *   8 mod 16), columns aligned to their element. */
uint64_t smj_dev_outer_join(smj_workspace * ws, const tuple_t * sortedR, uint64_t nR,
                            const tuple_t * sortedS, uint64_t nS, uint32_t keep,
                            int64_t * r_index_out   /* may be NULL */,
                            int64_t * s_index_out   /* may be NULL */,
                            value_t * r_payload_out /* may be NULL */,
                            value_t * s_payload_out /* may be NULL */,
                            intkey_t * key_out      /* may be NULL */,
                            uint64_t out_cap, smj_stream_t stream);

/* Its number of rows only, ADDED to *count_dev (device), stream-ordered like
 * smj_dev_band_join_count: no host synchronisation (the workspace's tables
 * grow on a first call).  The same keep and empty calls. */
void smj_dev_outer_join_count(smj_workspace * ws, const tuple_t * sortedR, uint64_t nR,
                              const tuple_t * sortedS, uint64_t nS, uint32_t keep,
                              unsigned long long * count_dev, smj_stream_t stream);

/* Grouped aggregation of a sorted relation: one output row per group, with
 * the group's first key, where it starts, how many tuples it holds and the
 * sum, minimum and maximum of their payloads (sort-based GROUP BY; the
 * library's own).  Two group tables give the per-key join cardinality
 * count_R[k] * count_S[k] without a join, and start/count are CSR offsets into
 * the sorted relation.  Total: there is no undefined input.
 * Group: a maximal run of consecutive tuples with equal key >> group_shift,
 *   an arithmetic shift of the key widened to int64, the group_shift of
 *   smj_dev_asof_join.  0 groups by key; values above 63 abort with a
 *   message.  On a relation with non-decreasing keys this is GROUP BY; on any
 *   other input it is the run-length form: keys 1,1,2,1 give three groups.
 *   Only the key order matters: the payloads of a run may come in any order
 *   (minimum and maximum are not taken from its first and last tuple).
 * Rows: row g belongs to the g-th group in input order.  key_out[g] is the
 *   key of the group's first tuple, start_out[g] that tuple's position in
 *   `sorted`, count_out[g] the number of tuples, sum_out[g] the sum of the
 *   payloads as int64 modulo 2^64 (two's complement wrap-around; the 8-byte
 *   library sign-extends its int32 payloads first), min_out[g] and max_out[g]
 *   their signed minimum and maximum.
 * Output: the first min(groups, out_cap) rows of every non-NULL column are
 *   written, everything else is left alone, and the number of groups is
 *   returned.  out_cap = 0, or all columns NULL, only counts.  Synchronises
 *   `stream` once, like smj_dev_band_join.
 * Empty call: n == 0 returns 0, launches nothing and does not synchronise.
 * Buffers: the input is left untouched; the outputs must not overlap it.
 *   Alignment as for the rest of the device API: any tuple-granular slice of a
 *   hipMalloc buffer (for the 8-byte library also one at an address that is
 *   8 mod 16), columns aligned to their element. */
uint64_t smj_dev_group_aggregate(smj_workspace * ws, const tuple_t * sorted, uint64_t n,
                                 uint32_t group_shift,
                                 intkey_t * key_out   /* may be NULL */,
                                 int64_t *  start_out /* may be NULL */,
                                 int64_t *  count_out /* may be NULL */,
                                 int64_t *  sum_out   /* may be NULL */,
                                 value_t *  min_out   /* may be NULL */,
                                 value_t *  max_out   /* may be NULL */,
                                 uint64_t out_cap, smj_stream_t stream);

/* Its number of groups only, ADDED to *groups_dev (device), stream-ordered
 * like smj_dev_band_join_count: no host synchronisation (the workspace's
 * tables grow on a first call).  The same groups; n == 0 adds nothing. */
void smj_dev_group_count(smj_workspace * ws, const tuple_t * sorted, uint64_t n,
                         uint32_t group_shift, unsigned long long * groups_dev,
                         smj_stream_t stream);

/* Elements of `sorted` one workgroup of the group kernels handles (for tests;
 * a host call, no device needed). */
uint32_t smj_group_tile(void);

/* Window functions over a sorted relation: one output row per tuple, the SQL
 * window functions over PARTITION BY key >> group_shift ORDER BY key with the
 * frame ROWS UNBOUNDED PRECEDING (the library's own).  Defined by position in
 * the input and total: there is no undefined input.
 * Heads: with g(i) = key[i] >> group_shift (an arithmetic shift of the key
 *   widened to int64; group_shift 0..63, values above 63 abort with a
 *   message), element i is a group head when i == 0 or g(i) != g(i-1), and a
 *   key head when i == 0 or key[i] != key[i-1].  Every group head is a key
 *   head.  h(i) is the last group head at or before i, p(i) the last key head
 *   at or before i.  On a relation with non-decreasing keys this is the SQL
 *   meaning; on any other input it is the run-length form: keys 1,1,2,1 give
 *   three groups.
 * Rows: every non-NULL column gets all n rows; row i belongs to sorted[i].
 *   group_out[i]      = the group heads in [0, i], minus 1: the row of
 *                       smj_dev_group_aggregate's table that holds i's group
 *                       (whole-group totals per tuple are a gather of that
 *                       table with this column).
 *   row_out[i]        = i - h(i)                 (ROW_NUMBER() - 1).
 *   rank_out[i]       = p(i) - h(i)              (RANK() - 1, ordered by key).
 *   dense_rank_out[i] = the key heads in (h(i), i]      (DENSE_RANK() - 1).
 *   sum_out[i]        = the sum of the payloads of sorted[h(i) .. i] as int64
 *                       modulo 2^64 (the 8-byte library sign-extends its int32
 *                       payloads first).
 *   min_out[i], max_out[i] = their signed minimum and maximum.
 *   Peers with equal keys do not share a value.  With group_shift == 0, rank
 *   and dense_rank are 0 everywhere (defined, not an error).
 * Output: nothing is written beyond row n - 1.  n == 0, or all seven columns
 *   NULL, launches nothing.  Stream-ordered like smj_dev_asof_join: no host
 *   synchronisation (the workspace's tables grow on a first call).
 * Buffers: the input is left untouched; the outputs must not overlap it or
 *   each other.  Alignment as for the rest of the device API: any
 *   tuple-granular slice of a hipMalloc buffer (for the 8-byte library also
 *   one at an address that is 8 mod 16), columns aligned to their element.
 *   n may exceed 2^32. */
void smj_dev_window(smj_workspace * ws, const tuple_t * sorted, uint64_t n,
                    uint32_t group_shift,
                    int64_t * group_out      /* may be NULL */,
                    int64_t * row_out        /* may be NULL */,
                    int64_t * rank_out       /* may be NULL */,
                    int64_t * dense_rank_out /* may be NULL */,
                    int64_t * sum_out        /* may be NULL */,
                    value_t * min_out        /* may be NULL */,
                    value_t * max_out        /* may be NULL */,
                    smj_stream_t stream);

/* Elements of `sorted` one workgroup of the window kernels handles (for
 * tests; a host call, no device needed). */
uint32_t smj_window_tile(void);

/* Sliding window frames over a sorted relation: one output row per tuple, the
 * SQL window aggregates over PARTITION BY key >> group_shift ORDER BY key with
 * the frame ROWS or RANGE BETWEEN lo AND hi around the tuple (the library's
 * own): rolling sums, minima and maxima over the last k rows or the last t
 * key units, LAG and LEAD, the group's total per tuple.  The work per row does
 * not depend on the frame's width.
 * Groups: smj_dev_window's.  h(i) is the last group head at or before i, e(i)
 *   the last position of i's group (one before the next group head, or n - 1).
 *   group_shift is 0..63; values above 63 abort with a message.
 * unit SMJ_FRAME_ROWS: the frame of row i is the positions j in [h(i), e(i)]
 *   with i + lo <= j <= i + hi, the sums taken without wrap-around.
 *   lo = INT64_MIN is UNBOUNDED PRECEDING, hi = INT64_MAX UNBOUNDED FOLLOWING.
 *   Total: defined by position on any input, the run-length form included.
 * unit SMJ_FRAME_RANGE: the frame of row i is the positions j in [h(i), e(i)]
 *   with key[i] + lo <= key[j] <= key[i] + hi.  The keys are widened to int64
 *   and the sums saturate at the ends of int64, exactly as in
 *   smj_dev_band_join; a band that lies wholly outside int64 is empty.  The
 *   band holds every peer (equal key) of i that it holds at all.  Requires
 *   non-decreasing keys inside each group; on other input the rows of such a
 *   group are unspecified, but the call still terminates, reads only
 *   sorted[0..n) and writes only rows 0..n-1.
 *   Any other unit aborts with a message.
 * Empty frames: lo > hi makes every frame empty; a frame can also be empty on
 *   its own (lo > 0 at a group's end, hi < 0 at its start, no key in the
 *   band).  An empty frame writes the library's NULL: -1 in start_out, 0 in
 *   every other column.
 * Rows: every non-NULL column gets all n rows; row i belongs to sorted[i].
 *   With the frame [a, b]:
 *   start_out[i] = a.
 *   count_out[i] = b - a + 1.
 *   sum_out[i]   = the sum of the payloads of sorted[a .. b] as int64 modulo
 *                  2^64 (the 8-byte library sign-extends its int32 payloads
 *                  first).
 *   min_out[i], max_out[i] = their signed minimum and maximum.
 *   first_out[i], last_out[i] = the payloads of sorted[a] and sorted[b].
 *   LAG(k) is first_out with ROWS lo = hi = -k, LEAD(k) with lo = hi = k, and
 *   the value is NULL where count_out is 0.  ROWS (INT64_MIN, 0) gives
 *   smj_dev_window's sum, minimum and maximum; RANGE (INT64_MIN, 0) is SQL's
 *   default frame, peers sharing the value of their last row; ROWS
 *   (INT64_MIN, INT64_MAX) is the group's total per tuple.
 * Output: nothing is written beyond row n - 1.  n == 0, or all seven columns
 *   NULL, launches nothing.  Stream-ordered like smj_dev_window: no host
 *   synchronisation (the workspace's tables grow on a first call).
 * Workspace: beside 64 bytes per 1024 tuples, a call holds per tuple 8 bytes
 *   for sum_out and, for each of min_out and max_out, 2 * sizeof(value_t) and
 *   another 3 * sizeof(value_t) per 64 tuples and (1 + log2(n / 1024)) *
 *   sizeof(value_t) per 1024: with all three columns about 25 bytes per tuple
 *   in the 8-byte library and 41 in the 16-byte one, and next to nothing for
 *   a call without them.
 * Buffers: the input is left untouched; the outputs must not overlap it or
 *   each other.  Alignment as for the rest of the device API: any
 *   tuple-granular slice of a hipMalloc buffer (for the 8-byte library also
 *   one at an address that is 8 mod 16), columns aligned to their element.
 *   n may exceed 2^32. */
#define SMJ_FRAME_ROWS  0u
#define SMJ_FRAME_RANGE 1u
void smj_dev_window_frame(smj_workspace * ws, const tuple_t * sorted, uint64_t n,
                          uint32_t group_shift, uint32_t unit, int64_t lo, int64_t hi,
                          int64_t * start_out /* may be NULL */,
                          int64_t * count_out /* may be NULL */,
                          int64_t * sum_out   /* may be NULL */,
                          value_t * min_out   /* may be NULL */,
                          value_t * max_out   /* may be NULL */,
                          value_t * first_out /* may be NULL */,
                          value_t * last_out  /* may be NULL */,
                          smj_stream_t stream);

/* Elements of `sorted` one workgroup of the frame kernels' write pass handles
 * (for tests; a host call, no device needed). */
uint32_t smj_frame_tile(void);

/* The inner aligned block of the frame kernels' range minimum and maximum: it
 * divides smj_frame_tile() (for tests; a host call, no device needed). */
uint32_t smj_frame_block(void);

/* The m-way join on one device.  R and S are left untouched; sortedR/sortedS
 * (n tuples each) receive the fully sorted relations; the match count is
 * written to *count_dev.  key_min <= key_max is an optional hint of the key
 * range (pass key_min > key_max to sample it on the device).  Asynchronous
 * except for one stream synchronisation that checks for skewed sub-buckets. */
void smj_dev_join(smj_workspace * ws, const tuple_t * R, uint64_t nR,
                  const tuple_t * S, uint64_t nS, tuple_t * sortedR,
                  tuple_t * sortedS, uint32_t fanout_bits, int64_t key_min,
                  int64_t key_max, unsigned long long * count_dev,
                  smj_stream_t stream);

/* Phase timings (ms) of the last smj_dev_join on this workspace, from HIP
 * events: [0]=partition [1]=tile pass [2]=bucket sort+join [3]=skew path
 * [4]=total. */
void smj_join_phase_ms(smj_workspace * ws, float * ms5);

/* Deterministic synthetic relations generated in HBM.
 * pk  : keys 1..total, each once (keyed bijection of the global index),
 *       payload 5 + global index (or 0 when with_payload == 0, as
 *       create_relation_pk leaves it);
 * fk  : keys perm(i) % maxid + 1 (uniform, |S| == maxid -> a permutation);
 * zipf: keys Zipf(theta) over 1..maxid, hot ranks spread by a bijection,
 *       payload 0.  `first` = global index of this shard's first tuple. */
void smj_dev_gen_pk(tuple_t * out, uint64_t n, uint64_t first, uint64_t total,
                    uint64_t seed, int with_payload, smj_stream_t stream);
void smj_dev_gen_fk(tuple_t * out, uint64_t n, uint64_t first, uint64_t total,
                    uint64_t maxid, uint64_t seed, smj_stream_t stream);
void smj_dev_gen_zipf(smj_workspace * ws, tuple_t * out, uint64_t n,
                      uint64_t first, uint64_t maxid, double theta,
                      uint64_t seed, smj_stream_t stream);

/* The reference's own rand()-driven generators, bit-exact (refgen.hip): the
 * relation create_relation_nonunique / create_relation_zipf would produce
 * after srand(seed) and `skip` earlier rand() calls (generator.c:220-231,
 * 490-505; genzipf.c:28-159, generator.c:517-534), shard [first, first + n) of
 * a relation of `total` tuples.  glibc rand()'s additive stream is jumped
 * ahead per shard (31 x 31 matrix powers); the Zipf alphabet and CDF table are
 * built on the host in the reference's order and cached per workspace.
 * nonunique: key = RAND_RANGE(maxid), payload = total - index, avoid_NaN;
 * zipf_ref : key = alphabet[CDF^-1(rand() / RAND_MAX)], payload 0
 *            (maxid < 2^32). */
void smj_dev_gen_nonunique(smj_workspace * ws, tuple_t * out, uint64_t n, uint64_t first,
                           uint64_t total, int64_t maxid, uint32_t seed, uint64_t skip,
                           smj_stream_t stream);
void smj_dev_gen_zipf_ref(smj_workspace * ws, tuple_t * out, uint64_t n, uint64_t first,
                          uint64_t maxid, double theta, uint32_t seed, uint64_t skip,
                          smj_stream_t stream);
/* The k-th rand() value after srand(seed) (k = 0 is the first call), by the
 * same jump-ahead, on the host (no device needed). */
uint32_t smj_glibc_rand(uint32_t seed, uint64_t k);

void smj_dev_synchronize(smj_stream_t stream);

/* Multi-GPU building block: partition of a device relation into 2^nbits key
 * ranges of [key_min, key_max] (monotone digits, unpadded, partitions back to
 * back; the order inside a partition is free: it is sorted afterwards), so a
 * caller can hand contiguous partition ranges to their owner GPU with one
 * all-to-all (bench.py does this over RCCL).  hist_out: device int64[2^nbits]. */
void smj_dev_partition_range(smj_workspace * ws, const tuple_t * in, uint64_t n,
                             tuple_t * out, uint32_t nbits, int64_t key_min,
                             int64_t key_max, int64_t * hist_out,
                             smj_stream_t stream);

/* Range partition of smj_dev_partition_range writing one 64-bit word per
 * tuple instead of the tuple (16-byte tuples only): word = (key offset inside
 * its partition, the low s1 bits) << (64 - s1) | payload, where partitions
 * cover 2^s1 keys.  Halves the bytes of the multi-GPU exchange.  Returns 0
 * (and launches nothing) when the layout does not apply -- the 8-byte
 * library, or partitions wider than 2^32 keys; otherwise 1, and *bad_flag is
 * OR-ed with 1 when some tuple cannot be packed (key outside [key_min,
 * key_max], payload outside [0, 2^(64 - s1))): the caller then partitions
 * the tuples instead. */
int smj_dev_partition_range_packed(smj_workspace * ws, const tuple_t * in, uint64_t n,
                                   uint64_t * out, uint32_t nbits, int64_t key_min,
                                   int64_t key_max, int64_t * hist_out,
                                   unsigned int * bad_flag, smj_stream_t stream);

/* Local join of one GPU's share after the exchange (multi-GPU join, no
 * reference counterpart: it replaces the per-thread multiway merge of the
 * reference's T>1 path, src/joins/sortmergejoin_multiway.c:463-556).  R and
 * S are the receive buffers: for every source GPU s in order, its range
 * partitions 0..2^bucket_bits-1 back to back, seg[s * 2^bucket_bits + b]
 * elements each (device int64).  Every partition b covers the keys
 * [key_lo + b * w, key_lo + (b + 1) * w) with 2^bucket_bits * w = 2^L, L the
 * bit length of key_hi - key_lo (any key_hi in [key_lo + 2^(L-1),
 * key_lo + 2^L - 1] gives the same plan), so the partitions are the level-1
 * buckets of the local sort: no local partition pass.  The elements are
 * tuples, or (flags & SMJ_SEG_PACKED) the words of
 * smj_dev_partition_range_packed for the same w.  R and S are used as
 * scratch (overwritten).  sortedR/sortedS receive the sorted relations as
 * tuples, count_dev the number of matching pairs. */
#define SMJ_SEG_PACKED 1u
/* Stages of one local join split over two calls with the same arguments
 * (the multi-GPU join overlaps them with the row exchange): a call with
 * SMJ_SEG_STAGE_R sorts only R's tiles (its tile pass: R must be complete,
 * S need not have arrived); the next call with SMJ_SEG_STAGE_REST sorts S's
 * tiles and runs the group pass and the count.  Neither flag: the whole join
 * in one call. */
#define SMJ_SEG_STAGE_R 2u
#define SMJ_SEG_STAGE_REST 4u
void smj_dev_join_segmented(smj_workspace * ws, void * R, uint64_t nR,
                            const int64_t * segR, void * S, uint64_t nS,
                            const int64_t * segS, uint32_t nseg,
                            uint32_t bucket_bits, int64_t key_lo, int64_t key_hi,
                            uint32_t flags, tuple_t * sortedR, tuple_t * sortedS,
                            unsigned long long * count_dev, smj_stream_t stream);

/* The local join of smj_dev_join_segmented from explicit segment tables:
 * bucket b (b < 2^bucket_bits) is the nseg segments startX/cntX[b * nseg + j]
 * (device int64, element offsets into X and element counts), so a receive
 * buffer may hold unused gaps between segments (the sampled exchange below).
 * nR / nS count the elements inside the segments. */
void smj_dev_join_segmented_tables(smj_workspace * ws, void * R, uint64_t nR,
                                   const int64_t * startR, const int64_t * cntR,
                                   void * S, uint64_t nS, const int64_t * startS,
                                   const int64_t * cntS, uint32_t nseg,
                                   uint32_t bucket_bits, int64_t key_lo, int64_t key_hi,
                                   uint32_t flags, tuple_t * sortedR, tuple_t * sortedS,
                                   unsigned long long * count_dev, smj_stream_t stream);

/* smj_dev_join_segmented_tables on 48-bit words in two planes (the layout
 * smj_dev_partition_range_planes writes): X's element i is
 * lo[i] | hi[i] << 32 with lo = (uint32_t *)X and hi = (uint16_t *)(lo +
 * strideX); strideX a multiple of 32 elements.  flags: the stage bits only.
 * Both tuple widths. */
void smj_dev_join_segmented_planes(smj_workspace * ws, void * R, uint64_t strideR,
                                   uint64_t nR, const int64_t * startR,
                                   const int64_t * cntR, void * S, uint64_t strideS,
                                   uint64_t nS, const int64_t * startS,
                                   const int64_t * cntS, uint32_t nseg,
                                   uint32_t bucket_bits, int64_t key_lo, int64_t key_hi,
                                   uint32_t flags, tuple_t * sortedR, tuple_t * sortedS,
                                   unsigned long long * count_dev, smj_stream_t stream);

/* Range partition of smj_dev_partition_range by the 1-GPU join's sampled
 * scatter (no histogram pass; packed words when `packed`).  Partition p is
 * smj_sampled_shards() consecutive regions, p's before p + 1's; region
 * i = p * shards + q holds seg_cnt[i] elements from element offset
 * seg_start[i] of `out` and is followed by unused slack, so `out` must hold
 * smj_sampled_capacity(n, nbits) elements (tuples, or 8-byte words).
 * flags (device uint32[2], zeroed here): [0] = 1 when a region overflowed
 * (the output is incomplete: use the exact partition), [1] = 1 when packed
 * and some tuple did not pack.  Returns 0 (nothing launched) when the form
 * does not apply: nbits > 10, n >= 2^32, or packed words unusable. */
int smj_dev_partition_range_sampled(smj_workspace * ws, const tuple_t * in, uint64_t n,
                                    void * out, uint32_t nbits, int64_t key_min,
                                    int64_t key_max, int packed, int64_t * seg_start,
                                    int64_t * seg_cnt, unsigned int * flags,
                                    smj_stream_t stream);
/* smj_dev_partition_range_sampled writing 48-bit words (both tuple widths,
 * the 1-GPU join's LayP48): w = (key - base) mod 2^s1 << (48 - s1) | payload,
 * s1 the partition width's bit count, payload as unsigned (8-byte tuples:
 * its 32 bits), stored as two planes of `out`: lo = w mod 2^32 at
 * (uint32_t *)out, hi = w >> 32 at (uint16_t *)((uint32_t *)out + stride);
 * stride >= smj_sampled_capacity(n, nbits), a multiple of 32.  flags[1]
 * gets 1 (payload wider than 64 - s1 bits), 2 (key outside the range) or 4
 * (payload wider than 48 - s1 bits), or-ed.  Returns 0 (nothing launched)
 * when the form does not apply: nbits > 10, n >= 2^32, or s1 outside 1..32. */
int smj_dev_partition_range_planes(smj_workspace * ws, const tuple_t * in, uint64_t n,
                                   void * out, uint64_t stride, uint32_t nbits,
                                   int64_t key_min, int64_t key_max, int64_t * seg_start,
                                   int64_t * seg_cnt, unsigned int * flags,
                                   smj_stream_t stream);
/* The same partition with exactly sized regions (round 6; the multi-GPU
 * exchange's form across ranks): one read pass counts every (partition,
 * shard), the regions are laid out back to back with no slack, so `out` needs
 * n elements and the partitions come out contiguous -- partition p is its
 * smj_sampled_shards() shard regions one after the other.  Tables and flags
 * as smj_dev_partition_range_sampled (the overflow flag stays 0).  Returns 0
 * when it does not apply (nbits > 10, n >= 2^32, packed words the plan does
 * not allow). */
int smj_dev_partition_range_shards(smj_workspace * ws, const tuple_t * in, uint64_t n,
                                   void * out, uint32_t nbits, int64_t key_min,
                                   int64_t key_max, int packed, int64_t * seg_start,
                                   int64_t * seg_cnt, unsigned int * flags,
                                   smj_stream_t stream);
uint64_t smj_sampled_capacity(uint64_t n, uint32_t nbits);
uint32_t smj_sampled_shards(void);

/* The multi-GPU exchange's tables (smj/dist.py; exchange.hip).  A rank's
 * range partition into F partitions of K shard regions (start/cnt: F x K
 * int64, exact partitions use shard 0; flags: uint32[2] = region overflow,
 * not packable, as smj_dev_partition_range_sampled writes them) goes to
 * `world` ranks: of the `used` partitions the plan's key range reaches
 * (0 = all F), partition p goes to rank p*world/used, and the partitions
 * from `used` on to the last rank (the ranks split the keys, not the
 * power-of-two partition space).
 * smj_dev_xsend writes the message to every rank g, rank after rank
 * ([chunk size, used elements, flags[1], flags[0], the owned regions'
 * offsets inside the chunk, their counts]: 4 + 2 K n_g int64 for n_g owned
 * partitions) and chunk[0..world) = chunk starts, chunk[world..2 world) =
 * chunk sizes.  smj_dev_xrecv takes the `world` messages received (each
 * 4 + 2 K mine int64) and writes the local join's segment tables (tstart,
 * tcnt: nbuckets x world*K, bucket-major; the rank's own chunk in place at
 * its chunk start, the others from element `cap` on, rank order) and
 * summary[4 world + 2] = chunk starts, chunk sizes (sends), receive sizes,
 * used elements received, the not-packable and overflow flags OR-ed over
 * the ranks. */
void smj_dev_xsend(const int64_t * start, const int64_t * cnt, const unsigned int * flags,
                   uint32_t F, uint32_t K, uint32_t world, uint32_t used, int64_t * msg,
                   int64_t * chunk, smj_stream_t stream);
void smj_dev_xrecv(const int64_t * msg, const int64_t * chunk, uint32_t world, uint32_t rank,
                   uint32_t mine, uint32_t K, uint32_t nbuckets, uint64_t cap,
                   int64_t * tstart, int64_t * tcnt, int64_t * summary, smj_stream_t stream);

/* Self-check of the hardware property behind the stable partition's ranks:
 * LDS atomic adds return their old values to the lanes of one instruction
 * that hit the same word in lane order (partition.hip, k_scatter_swp).
 * Returns the number of violations (0 expected; synchronises `stream`).  The
 * library runs it once per process before its first stable partition and
 * falls back to ballot ranks on a device without the property. */
uint64_t smj_selfcheck_lds_order(smj_workspace * ws, smj_stream_t stream);

/* The calling thread's workspace behind the reference-named entry points
 * (sortmergejoin_multiway, avxsort_tuples, ...): lets a caller trace their
 * kernels with smj_trace_* (bench.py --api). */
smj_workspace * smj_context_workspace(void);

/* Per-kernel HIP-event trace of the join pipeline (bench.py roofline). */
void smj_trace_enable(smj_workspace * ws, int on);
void smj_trace_reset(smj_workspace * ws);
/* Trace only the kernel `name` (NULL or "": every kernel): one event pair per
 * step instead of one per kernel in bench.py's timed loop. */
void smj_trace_only(smj_workspace * ws, const char * name);
int smj_trace_read(smj_workspace * ws, char * names, int cap, float * ms_sum,
                   int * launches, int max);

#ifdef __cplusplus
}
#endif
#endif /* SMJ_H */
