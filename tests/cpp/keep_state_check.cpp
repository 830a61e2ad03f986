// Host-side check of the keep mask's per-chunk helpers (csrc/rtr_chunk_box.h): rtr::keep_chunk_state against a
// point-by-point count of the chunk's kept points below n, and rtr::keep_lane_bits against the bit layout of the mask
// (lane l of a chunk: points 4 l .. 4 l + 3 = bits (l % 8) * 4 .. + 3 of the chunk's word l / 8).  Random words, every
// valid count 1..256, sparse and dense words, and words with bits set past the valid count (which must not count).
// Prints "ok <chunks> <none> <all> <some>".
#include <cstdint>
#include <cstdio>
#include <random>

#include "rtr_chunk_box.h"

int main() {
    std::mt19937_64 rng(0x4EE9u);
    long chunks = 0, cnt[3] = {0, 0, 0};
    for (int t = 0; t < 300000; ++t) {
        uint32_t w[8];
        const int kind = (int)(rng() % 6);
        for (int j = 0; j < 8; ++j) {
            uint32_t v = (uint32_t)rng();
            if (kind == 0) v = 0u;
            if (kind == 1) v = 0xFFFFFFFFu;
            if (kind == 2) v = 1u << (rng() % 32);
            if (kind == 3) v = ~(1u << (rng() % 32));
            w[j] = v;
        }
        if (kind == 4) {  // all kept below a random count, random above it
            for (int j = 0; j < 8; ++j) w[j] = 0xFFFFFFFFu;
            w[rng() % 8] = (uint32_t)rng();
        }
        const uint32_t valid = (t % 4 == 0) ? 256u : 1u + (uint32_t)(rng() % 256);
        int kept = 0;
        for (uint32_t p = 0; p < valid; ++p) kept += (w[p / 32] >> (p % 32)) & 1u;
        const uint8_t want = kept == 0 ? rtr::kKeepNone : (kept == (int)valid ? rtr::kKeepAll : rtr::kKeepSome);
        const uint8_t got = rtr::keep_chunk_state(w, valid);
        if (got != want) {
            printf("state mismatch: t %d valid %u kept %d got %d want %d\n", t, valid, kept, got, want);
            return 1;
        }
        ++cnt[got];
        ++chunks;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            uint32_t want_bits = 0;
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t p = 4 * lane + k;
                want_bits |= ((w[p / 32] >> (p % 32)) & 1u) << k;
            }
            if (rtr::keep_lane_bits(w[lane / 8], lane) != want_bits) {
                printf("lane bits mismatch: t %d lane %u\n", t, lane);
                return 1;
            }
        }
    }
    printf("ok %ld %ld %ld %ld\n", chunks, cnt[rtr::kKeepNone], cnt[rtr::kKeepAll], cnt[rtr::kKeepSome]);
    return 0;
}
