// C entry points over csrc/partition_policy.hpp for
// tests/test_partition_policy.py.  Scatters cross as the enum's integers.
#include "../../avx-sort-merge-joins_amd/csrc/partition_policy.hpp"

using namespace smj;

extern "C" {

int pp_stable_scatter_choice(uint64_t n, uint32_t dbits, uint32_t tb, int lds_order_ok,
                             int forced) {
    return (int)stable_scatter_choice(n, dbits, tb, lds_order_ok != 0, forced != 0);
}

int pp_ballot_scatter_choice(uint32_t dbits, uint32_t tb) {
    return (int)ballot_scatter_choice(dbits, tb);
}

uint64_t pp_swa_lds_bytes(uint32_t threads, uint32_t items, uint32_t tb, uint32_t nbins) {
    return swa_lds_bytes(threads, items, tb, nbins);
}

uint64_t pp_swc_lds_bytes(uint32_t threads, uint32_t items, uint32_t tb, uint32_t nbins) {
    return swc_lds_bytes(threads, items, tb, nbins);
}

uint32_t pp_swc_max_segs(uint32_t threads, uint32_t items, uint32_t tb, uint32_t nbins) {
    return swc_max_segs(threads, items, tb, nbins);
}

uint64_t pp_scatter_lds_bytes(uint32_t threads, uint32_t items, uint32_t tb, uint32_t nbins) {
    return scatter_lds_bytes(threads, items, tb, nbins);
}

uint32_t pp_swp_items(uint32_t tb) { return swp_items(tb); }
uint64_t pp_lds_limit(void) { return kScatterLdsLimit; }
uint32_t pp_scatter_bit(int scatter) { return scatter_bit((Scatter)scatter); }
uint32_t pp_two_pass_bit(void) { return kScatterTwoPass; }

}  // extern "C"
