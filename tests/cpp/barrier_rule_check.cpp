// The wait condition of the peer-to-peer flag barrier (csrc/rtr_barrier_rule.h) built with plain g++.
//
// not_arrived(flag, seq): the peer whose flag word reads `flag` has not yet reached barrier `seq`; both are 32-bit
// counters that wrap.  Checked:
//   1. wherever neither value has wrapped it is `flag < seq` (within the 2^31 a serial-number comparison tells apart);
//   2. a flag up to 2^31 - 1 behind still waits, across 0xFFFFFFFF -> 0 (seq small again, flag still large);
//   3. a flag at or ahead of seq never waits, across the wrap too (a peer may be one barrier ahead);
//   4. a counter walked through the wrap as the library drives it (++seq per barrier, the peer's flag the barrier
//      before): every barrier waits for the late peer and lets the arrived one through.
// With -DBARRIER_RULE_OLD the predicate is the comparison the kernels used before, `flag < seq`: the program must then
// FAIL (it prints "FAIL ..." and returns 1) -- tests/test_cpp_wrap_rules.py builds both and asserts both outcomes, so
// the old rule's defect is shown here, on the host.
// Prints "ok <checks>".
#include <cstdio>

#include "rtr_barrier_rule.h"

#ifdef BARRIER_RULE_OLD
static bool not_arrived(uint32_t flag, uint32_t seq) { return flag < seq; }
#else
static bool not_arrived(uint32_t flag, uint32_t seq) { return rtr::barrier_not_arrived(flag, seq); }
#endif

static long long checks = 0;
#define CHECK(cond)                                             \
    do {                                                        \
        ++checks;                                               \
        if (!(cond)) {                                          \
            printf("FAIL line %d: %s\n", __LINE__, #cond);      \
            return 1;                                           \
        }                                                       \
    } while (0)

int main() {
    const uint32_t kHalf = 0x80000000u;
    // distances worth looking at: the near ones every barrier sees, powers of two, the last one the comparison tells apart
    uint32_t dist[80];
    int nd = 0;
    for (uint32_t d = 1; d <= 16; ++d) dist[nd++] = d;
    for (int b = 5; b < 31; ++b) dist[nd++] = 1u << b, dist[nd++] = (1u << b) + 1u;
    dist[nd++] = kHalf - 2u, dist[nd++] = kHalf - 1u;
    // counter values: the start, the middle of the range, both sides of the wrap
    const uint32_t seqs[] = {0u, 1u, 2u, 17u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFF0u, 0xFFFFFFFEu, 0xFFFFFFFFu};

    // 1. no wrap between the two: the plain comparison
    for (uint32_t seq : seqs)
        for (int i = 0; i < nd; ++i) {
            const uint32_t d = dist[i];
            if (seq >= d) CHECK(not_arrived(seq - d, seq) == (seq - d < seq));               // flag behind, not wrapped
            if (seq <= 0xFFFFFFFFu - d) CHECK(not_arrived(seq + d, seq) == (seq + d < seq));  // flag ahead, not wrapped
            CHECK(not_arrived(seq, seq) == false);
        }
    // 2. behind by 1 .. 2^31 - 1 waits, wherever the two lie -- in particular seq just past the wrap, flag before it
    for (uint32_t seq : seqs)
        for (int i = 0; i < nd; ++i) CHECK(not_arrived(seq - dist[i], seq));
    for (uint32_t seq = 0; seq < 64; ++seq)
        for (uint32_t d = seq + 1; d < seq + 64; ++d) CHECK(not_arrived(seq - d, seq));  // (flag = 0xFFFFFF.., seq small)
    // 3. at or ahead of seq (by less than 2^31) never waits
    for (uint32_t seq : seqs) {
        CHECK(!not_arrived(seq, seq));
        for (int i = 0; i < nd; ++i) CHECK(!not_arrived(seq + dist[i], seq));
    }
    for (uint32_t seq = 0xFFFFFFC0u; seq != 0; ++seq)
        for (uint32_t d = 0; d < 128; ++d) CHECK(!not_arrived(seq + d, seq));  // (flag small again, seq still large)
    // 4. the counter as the library drives it, from 0xFFFFFFF0 through 0 (what the GPU tests start from)
    uint32_t q = 0xFFFFFFF0u;
    for (int k = 0; k < 64; ++k) {
        const uint32_t before = q;
        ++q;                              // this rank enters barrier q
        CHECK(not_arrived(before, q));    // a peer still at the previous barrier: wait
        CHECK(!not_arrived(q, q));        // arrived
        CHECK(!not_arrived(q + 1u, q));   // already in the next one
        CHECK(not_arrived(q - 3u, q));    // a stalled peer, three barriers back: wait (and time out)
    }
    CHECK(q == 0x30u);
    printf("ok %lld\n", checks);
    return 0;
}
