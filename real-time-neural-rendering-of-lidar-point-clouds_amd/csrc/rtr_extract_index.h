// rtr_extract_index.h -- the window arithmetic of rtr_extract_points (rtr.h section 2e), shared by its kernel and the
// host (plain C++ apart from the qualifiers: tests/cpp/extract_index_check.cpp compiles it with g++ and fuzzes it).
#pragma once
#include <stdint.h>

#include "rtr_remove_index.h"

namespace rtr {

// The selected upload indices in ascending order are s_0 < s_1 < ... < s_{k-1}; a call (or one internal window of it)
// produces the ranks [first, first + count) into slots 0 .. count - 1.  The rank of a selected point u is remove_rank's:
// the set bits of the selection below u.

// The bits of selection word w that name points below n (bits at or past n are ignored).
RTR_HD uint32_t extract_word_mask(uint64_t w, uint64_t n) {
    const uint64_t lo = w * 32u;
    if (lo >= n) return 0u;
    return n - lo >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)(n - lo)) - 1u;
}

// Rank -> output slot; false: the rank lies outside the window.  (first + count may pass 2^64: no such sum is formed.)
RTR_HD bool extract_slot(uint64_t rank, uint64_t first, uint64_t count, uint64_t *slot) {
    if (rank < first || rank - first >= count) return false;
    *slot = rank - first;
    return true;
}

// A 256-point chunk of a cloud in upload order owns the contiguous ranks [run_lo, run_hi): run_lo = the exclusive
// popcount scan at its first word, run_hi = the scan at the next chunk's first word (the total behind the last chunk).
// True: none of them falls in the window, the chunk is skipped before anything of it is read.
RTR_HD bool extract_chunk_skip(uint64_t run_lo, uint64_t run_hi, uint64_t first, uint64_t count) {
    if (run_hi <= run_lo || count == 0u) return true;       // no selected point / nothing asked for
    if (run_hi <= first) return true;                       // wholly before the window
    return run_lo >= first && run_lo - first >= count;      // wholly behind it
}

// The chunks [c0, c1) that hold the ranks of the window when EVERY point is extracted in the resident order (rank =
// resident index): c0 = first / 256, c1 = one past the chunk of the last rank.  count > 0, first + count <= n.
RTR_HD void extract_all_chunks(uint64_t first, uint64_t count, uint64_t *c0, uint64_t *c1) {
    *c0 = first / 256u;
    *c1 = (first + count - 1u) / 256u + 1u;
}

}  // namespace rtr
