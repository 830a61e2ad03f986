// rtr_write_index.h -- the window arithmetic of rtr_write_points (rtr.h section 2f), shared by its kernel and the host
// (plain C++ apart from the qualifiers: tests/cpp/write_index_check.cpp compiles it with g++ and fuzzes it).
#pragma once
#include <stdint.h>

#include "rtr_extract_index.h"

namespace rtr {

// The selected upload indices in ascending order are s_0 < s_1 < ... < s_{k-1}; a call writes the points of ranks
// [first, first + count).  The bits of selection word w (`word`, scan = the exclusive popcount scan at w: the selected
// points below 32 w) that name such a point: bits at or past n are dropped (extract_word_mask), a bit's rank is
// remove_rank's and the window test extract_slot's, which forms no sum that can pass 2^64.
RTR_HD uint32_t write_word_bits(uint32_t word, uint32_t scan, uint64_t w, uint64_t first, uint64_t count, uint64_t n) {
    const uint32_t live = word & extract_word_mask(w, n);
    uint32_t out = 0u;
    for (uint32_t rest = live; rest; rest &= rest - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctz(rest);
        uint64_t slot;
        if (extract_slot(remove_rank(scan, live, b), first, count, &slot)) out |= 1u << b;
    }
    return out;
}

}  // namespace rtr
