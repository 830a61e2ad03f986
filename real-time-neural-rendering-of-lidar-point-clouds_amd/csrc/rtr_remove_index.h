// rtr_remove_index.h -- the index arithmetic of rtr_remove_points (rtr.h section 2c), shared by its kernels and the
// host (plain C++ apart from the qualifiers: tests/cpp/remove_index_check.cpp compiles it with g++ and fuzzes it).
#pragma once
#include <stdint.h>

#ifndef RTR_HD
#if defined(__HIPCC__)
#define RTR_HD __host__ __device__ inline
#else
#define RTR_HD inline
#endif
#endif

namespace rtr {

// Upload-order keep words: bit u % 32 of word u / 32 set = point u stays.  Survivor u gets the new index rank(u), the
// number of kept points below u: scan = the exclusive sum of the popcounts of the words before word u / 32.
RTR_HD uint32_t remove_rank(uint32_t scan, uint32_t word, uint32_t u) {
    return scan + (uint32_t)__builtin_popcount(word & ((1u << (u & 31u)) - 1u));
}

// A 256-point chunk, one wave: lane l holds its points 4 l + k (k = 0..3), ballot[k] bit l = point 4 l + k stays.  The
// survivors keep their order; the one at 4 l + k lands at slot `below` + popc(own & ((1 << k) - 1)) of the chunk, below
// = the survivors of lanes < l (remove_lane_below on the host; the kernel counts them with a chained
// mbcnt_lo / mbcnt_hi over the four ballots instead, a form only the GPU equivalence tests, tests/test_gpu_remove.py,
// exercise -- the g++ fuzz checks this stand-in) and own = lane l's four bits (remove_lane_bits).
RTR_HD uint32_t remove_lane_bits(const uint64_t ballot[4], uint32_t lane) {
    uint32_t b = 0;
    for (uint32_t k = 0; k < 4; ++k) b |= (uint32_t)((ballot[k] >> lane) & 1u) << k;
    return b;
}
RTR_HD uint32_t remove_lane_below(const uint64_t ballot[4], uint32_t lane) {
    const uint64_t m = lane >= 64u ? ~0ull : ((1ull << lane) - 1ull);
    uint32_t s = 0;
    for (uint32_t k = 0; k < 4; ++k) s += (uint32_t)__builtin_popcountll(ballot[k] & m);
    return s;
}
RTR_HD uint32_t remove_slot(uint32_t below, uint32_t own, uint32_t k) {
    return below + (uint32_t)__builtin_popcount(own & ((1u << k) - 1u));
}

// The bits of `mask` at the set bits of `keep`, packed to the bottom in order (a parallel bit extract): the compacted
// keep mask in force takes them at bit rank(first kept point of the word) on.
RTR_HD uint32_t remove_extract(uint32_t mask, uint32_t keep) {
    uint32_t out = 0, j = 0;
    while (keep) {
        const uint32_t low = keep & (0u - keep);
        out |= (mask & low) ? (1u << j) : 0u;
        ++j;
        keep ^= low;
    }
    return out;
}

}  // namespace rtr
