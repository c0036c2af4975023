#pragma once
// partition_policy.hpp -- which scatter kernel a stable partition of up to
// kNarrowDigitBits digit bits launches, and the LDS sizes the choice rests on.
// Plain host C++ (no HIP headers): the launches live in partition.hip
// (stable_partition_narrow, partition_hist_scatter), the decision here, driven
// on the CPU by tests/test_partition_policy.py through tests/partition_host.
//
//   atomic        k_scatter_swp<512, 8 or 16>: ranks from lane-ordered LDS
//                 atomics, 32-bit positions, one workgroup a CU
//   ballot-wc     k_scatter_swc<512, 8> on the counts of k_hist<512, 16>:
//                 ballot ranks, whole-segment stores, carries in LDS
//   ballot-512x16 k_scatter<512, 16>: ballot ranks, plain stores
//   ballot-256x8  k_scatter<256, 8>: the same on small tiles (digits of 11 and
//                 12 bits, whose per-wave counters need the LDS)
#include <stddef.h>
#include <stdint.h>

namespace smj {

enum class Scatter : int { Atomic = 0, BallotWc = 1, Ballot512x16 = 2, Ballot256x8 = 3 };
// bits of Workspace::last_scatter (SMJ_SCATTER_* of smj.h; capi.hip asserts
// it): 1 << Scatter, and the two stable passes of a digit wider than 12 bits
constexpr uint32_t kScatterTwoPass = 16;
constexpr uint32_t scatter_bit(Scatter s) { return 1u << (int)s; }

// what a workgroup may ask for (gfx950: 160 KiB a CU)
constexpr size_t kScatterLdsLimit = 160 * 1024;
// k_scatter_swp keeps output positions in 32 bits
constexpr uint64_t kSwpPositions = 1ull << 32;

// --- k_scatter_swp (SwaGeom): stage Tup[TILE] | carry Tup[B][SEG - 1] |
// counters u32[W][B / 2] | info u32x4[B] | segown u16[TILE / SEG + 2 B] |
// scan scratch; SEG tuples of tb bytes fill a segment of seg_bytes
constexpr size_t swa_lds_bytes(uint32_t threads, uint32_t items, uint32_t tb, uint32_t B,
                               uint32_t seg_bytes = 64) {
    return (size_t)threads * items * tb + (size_t)B * (seg_bytes / tb - 1) * tb +
           (size_t)(threads / 64) * B * 2 + (size_t)B * 16 +
           ((size_t)(threads * items / (seg_bytes / tb) + 2 * B) * 2 + 15) / 16 * 16 + 128;
}

// --- k_scatter_swc (SwcGeom): segments a tile can emit: its own tuples and
// every digit's carry in whole segments, plus a partial first and last one a
// digit
constexpr uint32_t swc_max_segs(uint32_t threads, uint32_t items, uint32_t tb, uint32_t nbins) {
    return (threads * items + nbins * (64 / tb - 1)) / (64 / tb) + 2 * nbins;
}
// stage Tup[TILE] | carry Tup[nbins * (SEG - 1)] | run u64[nbins] |
// tstart, kc, segpre, emit u32[nbins] | wcnt u16[WAVES * nbins] |
// segown u16[max_segs] | scan scratch
constexpr size_t swc_lds_bytes(uint32_t threads, uint32_t items, uint32_t tb, uint32_t nbins) {
    return (size_t)threads * items * tb + (size_t)nbins * (64 / tb - 1) * tb +
           (size_t)nbins * (8 + 4 * 4) + (size_t)(threads / 64) * nbins * 2 +
           ((size_t)swc_max_segs(threads, items, tb, nbins) * 2 + 15) / 16 * 16 + 64;
}

// --- k_scatter: stage Tup[TILE] | run u64[nbins] | tstart u32[nbins] |
// wcnt u16[WAVES * nbins] | scan scratch
constexpr size_t scatter_lds_bytes(uint32_t threads, uint32_t items, uint32_t tb,
                                   uint32_t nbins) {
    return (size_t)threads * items * tb + (size_t)nbins * 8 + (size_t)nbins * 4 +
           (size_t)(threads / 64) * nbins * 2 + 64;
}

// items a lane of k_scatter_swp: 64 KiB of tuples a tile at either width
constexpr uint32_t swp_items(uint32_t tb) { return tb == 16 ? 8 : 16; }

// The ballot-rank kernels (partition_hist_scatter<.., STABLE = true>): write
// combining where its 512 x 8 geometry fits (the per-digit scans of
// k_scatter_swc give a thread up to four digits), else the plain scatter on
// the histogram's own tiles.
inline Scatter ballot_scatter_choice(uint32_t dbits, uint32_t tb) {
    const uint32_t nbins = 1u << dbits;
    if (nbins <= 4 * 512 && swc_lds_bytes(512, 8, tb, nbins) <= kScatterLdsLimit)
        return Scatter::BallotWc;
    // the big tiles need the 16-bit per-wave counters and <= 160 KiB LDS
    return dbits <= 10 ? Scatter::Ballot512x16 : Scatter::Ballot256x8;
}

// The scatter of one stable pass over n tuples of tb bytes at dbits digit
// bits (0..12).  lds_order_ok: the device returns the old values of colliding
// LDS atomics in lane order (smj_selfcheck_lds_order); forced:
// smj_workspace_force_ballot_ranks, which answers as if it did not.
inline Scatter stable_scatter_choice(uint64_t n, uint32_t dbits, uint32_t tb, bool lds_order_ok,
                                     bool forced, uint32_t swp_seg_bytes = 64) {
    // positions are 32-bit inside k_scatter_swp; its LDS holds 2^10 digits
    if (dbits >= 1 && dbits <= 10 && n + ((uint64_t)64 << dbits) < kSwpPositions &&
        swa_lds_bytes(512, swp_items(tb), tb, 1u << dbits, swp_seg_bytes) <= kScatterLdsLimit &&
        lds_order_ok && !forced)
        return Scatter::Atomic;
    return ballot_scatter_choice(dbits, tb);
}

}  // namespace smj
