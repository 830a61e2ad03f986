// The index arithmetic of rtr_remove_points (csrc/rtr_remove_index.h) built with plain g++ and fuzzed against a
// point-by-point reference: the renumbering rank, a survivor's slot in its chunk from the four ballots, and the bit
// extract that compacts the keep mask in force.  Prints "ok <chunks> <words>".
#include <cstdio>
#include <random>
#include <vector>

#include "rtr_remove_index.h"

static int fail(const char* what, unsigned long long a, unsigned long long b) {
    printf("FAIL %s %llu %llu\n", what, a, b);
    return 1;
}

int main() {
    std::mt19937_64 rng(0x5EED0001ull);
    // survivor slots: random keep patterns over 256-point chunks (lane l holds points 4 l .. 4 l + 3)
    const int chunks = 20000;
    for (int t = 0; t < chunks; ++t) {
        const int mode = t % 5;  // dense, sparse, all, none, random density
        const double p = mode == 0 ? 0.9 : mode == 1 ? 0.05 : mode == 2 ? 1.0 : mode == 3 ? 0.0 : (rng() % 1001) / 1000.0;
        std::bernoulli_distribution keep(p);
        bool k[256];
        uint64_t ballot[4] = {0, 0, 0, 0};
        for (int i = 0; i < 256; ++i) {
            k[i] = keep(rng);
            if (k[i]) ballot[i % 4] |= 1ull << (i / 4);
        }
        uint32_t next = 0;  // the reference: survivors in order
        for (int i = 0; i < 256; ++i) {
            if (!k[i]) continue;
            const uint32_t lane = (uint32_t)(i / 4), kk = (uint32_t)(i % 4);
            const uint32_t own = rtr::remove_lane_bits(ballot, lane);
            const uint32_t slot = rtr::remove_slot(rtr::remove_lane_below(ballot, lane), own, kk);
            if (slot != next) return fail("slot", (unsigned long long)i, slot);
            ++next;
        }
        if (rtr::remove_lane_below(ballot, 64) != next) return fail("count", next, rtr::remove_lane_below(ballot, 64));
    }
    // ranks and the compacted mask over random upload-order words
    const int words = 200000;
    std::vector<uint32_t> kw(words), mw(words);
    for (int w = 0; w < words; ++w) {
        const int mode = w % 7;
        kw[w] = mode == 0 ? 0xFFFFFFFFu : mode == 1 ? 0u : mode == 2 ? (uint32_t)(rng() & rng()) : (uint32_t)rng();
        mw[w] = (uint32_t)rng();
    }
    std::vector<uint32_t> ref_rank;  // rank of every kept point, and the compacted mask bit by bit
    std::vector<uint8_t> ref_mask;
    uint32_t scan = 0;
    std::vector<uint32_t> packed((size_t)words + 1, 0u);
    for (int w = 0; w < words; ++w) {
        const uint32_t before = scan;
        for (uint32_t b = 0; b < 32; ++b) {
            const uint32_t u = (uint32_t)w * 32u + b;
            if (!((kw[w] >> b) & 1u)) continue;
            const uint32_t r = rtr::remove_rank(before, kw[w], u);
            if (r != scan) return fail("rank", u, r);
            ref_mask.push_back((uint8_t)((mw[w] >> b) & 1u));
            ++scan;
        }
        // the kernel's scatter of the extracted bits at bit `before`
        const uint32_t bits = rtr::remove_extract(mw[w], kw[w]);
        const uint32_t cnt = (uint32_t)__builtin_popcount(kw[w]);
        if (cnt < 32 && (bits >> cnt)) return fail("extract width", (unsigned long long)w, bits);
        const uint32_t sh = before & 31u;
        packed[before >> 5] |= bits << sh;
        if (sh && (bits >> (32u - sh))) packed[(before >> 5) + 1] |= bits >> (32u - sh);
    }
    for (size_t i = 0; i < ref_mask.size(); ++i)
        if (((packed[i / 32] >> (i % 32)) & 1u) != ref_mask[i]) return fail("mask", i, ref_mask[i]);
    for (size_t i = ref_mask.size(); i < (size_t)words * 32; ++i)
        if ((packed[i / 32] >> (i % 32)) & 1u) return fail("mask tail", i, 1);
    printf("ok %d %d\n", chunks, words);
    return 0;
}
