// rtr_topk_cascade.h -- the k smallest of a stream of distinct 64-bit keys, kept in a row of k slots by any number of
// writers at once with nothing but a fetch-min: no compare-and-swap loop, no lock, no retry, and no writer ever waits for
// another.  rtr_nearest_k.hip (rtr_nearest_k_points, rtr.h section 6m) runs it on global memory with the returning 64-bit
// atomicMin; tests/cpp/topk_cascade_check.cpp runs these very lines on std::atomic from several threads.
//
// A row starts as k slots of all ones (kTopkEmpty, above every key).  To insert a key, walk the row from slot 0: at each
// slot, old = fetch_min(slot, key), and carry max(old, key) on; stop when the carried key is all ones or the row ends.
//   Each slot ends as the minimum of everything that ever reached it.  Slot 0 is reached by every key.  A step leaves the
//   smaller of (old, key) in the slot and passes the larger on, so of the keys that reach slot s exactly one -- in the
//   end the smallest -- stays behind and all others reach slot s + 1: slot s + 1 is reached by every key but the s + 1
//   smallest.  At quiescence row[s] is therefore the (s + 1)-th smallest key, for any interleaving of the writers; slots
//   past the number of keys still hold all ones.  (The keys must be distinct: two equal keys would leave one behind and
//   lose the other.)
// The PRUNE: a slot only ever decreases, and row[k - 1] = v means that v was the larger at each of the k - 1 slots before,
// so k - 1 distinct keys below v exist already.  A key >= ANY earlier read of row[k - 1], however stale, is hence not
// among the final k and may be dropped without touching memory (topk_beats).
// The SKIP: a step at a slot that holds less than the key changes nothing -- the minimum leaves the slot as it is, and the
// larger of the two, the key, is carried on.  A slot only ever decreases, so a slot that was READ below the key at any
// earlier time, however stale, still holds less when the key would get there: the walk may start behind a run of such
// slots (`first`) and the row ends the same.  Of a row that is full this saves the steps before the key's own place.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTR_TOPK_HD __host__ __device__
#else
#define RTR_TOPK_HD
#endif

namespace rtr {

constexpr uint64_t kTopkEmpty = ~0ull;

// may `key` still be among the k smallest, given `bound`, a read of row[k - 1] at any earlier time?
RTR_TOPK_HD inline bool topk_beats(uint64_t key, uint64_t bound) { return key < bound; }

// Inserts `key` into a row of k slots.  fetch_min(s, v): row[s] = min(row[s], v) atomically, returning what row[s] held
// before.  A key of all ones inserts nothing.  first: the slot to start at -- every slot before it was read below `key`
// (see "The SKIP"); 0 when nothing was read.  Returns the number of fetch_min calls made.
template <class FetchMin>
RTR_TOPK_HD inline uint32_t topk_cascade(uint32_t k, uint64_t key, FetchMin &&fetch_min, uint32_t first = 0) {
    uint32_t s = first, calls = 0;
    for (; s < k && key != kTopkEmpty; ++s, ++calls) {
        const uint64_t old = fetch_min(s, key);
        key = old > key ? old : key;
    }
    return calls;
}

}  // namespace rtr
