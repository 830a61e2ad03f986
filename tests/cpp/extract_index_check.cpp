// The window arithmetic of rtr_extract_points (csrc/rtr_extract_index.h) built with plain g++ and fuzzed against a plain
// loop that ranks the set bits: the tail word's mask, rank -> slot, and the chunk-run rejection, which must never be
// given for a chunk that owns a rank of the window.  Prints "ok <cases> <chunks skipped> <chunks kept> <points placed>".
#include <cstdio>
#include <random>
#include <vector>

#include "rtr_extract_index.h"

static int fail(const char* what, unsigned long long a, unsigned long long b, unsigned long long c) {
    printf("FAIL %s %llu %llu %llu\n", what, a, b, c);
    return 1;
}

int main() {
    std::mt19937_64 rng(0x5EED0015ull);
    unsigned long long cases = 0, skipped = 0, kept_chunks = 0, placed = 0;
    const int selections = 25000, windows = 40;
    std::vector<uint32_t> words, scan, written;
    std::vector<uint64_t> ranked;  // the reference: the selected points in ascending order
    for (int t = 0; t < selections; ++t) {
        // n: not a multiple of 32 or 256 most of the time, sometimes exactly one
        uint64_t n = 1 + rng() % (t % 8 == 0 ? 2100 : 700);
        if (t % 11 == 0) n = 256 * (1 + rng() % 4);
        if (t % 13 == 0) n = 32 * (1 + rng() % 20);
        const uint64_t nwords = (n + 31) / 32, nch = (n + 255) / 256;
        const int mode = t % 6;  // dense, sparse, all, none, random words, runs
        words.assign(nwords, 0u);
        for (uint64_t w = 0; w < nwords; ++w) {
            uint32_t v = (uint32_t)rng();
            if (mode == 0) v |= (uint32_t)rng() | (uint32_t)rng();
            else if (mode == 1) v &= (uint32_t)rng() & (uint32_t)rng() & (uint32_t)rng();
            else if (mode == 2) v = 0xFFFFFFFFu;
            else if (mode == 3) v = 0u;
            else if (mode == 5) v = ((w / 9) % 2) ? 0xFFFFFFFFu : 0u;
            words[w] = v;
        }
        if (mode != 3 || t % 2) words[nwords - 1] |= ~rtr::extract_word_mask(nwords - 1, n);  // garbage bits past n (none when n % 32 == 0)
        // the reference ranking and the scan the device builds (the tail word masked)
        ranked.clear();
        for (uint64_t u = 0; u < n; ++u)
            if ((words[u / 32] >> (u % 32)) & 1u) ranked.push_back(u);
        scan.assign(nwords, 0u);
        uint32_t run = 0;
        for (uint64_t w = 0; w < nwords; ++w) {
            scan[w] = run;
            uint32_t m = rtr::extract_word_mask(w, n), ref = 0;
            for (uint32_t b = 0; b < 32; ++b) ref |= (w * 32 + b < n) ? 1u << b : 0u;
            if (m != ref) return fail("word mask", w, n, m);
            run += (uint32_t)__builtin_popcount(words[w] & m);
        }
        const uint64_t k = ranked.size();
        if (run != k) return fail("total", run, k, n);
        if (rtr::extract_word_mask(nwords, n) != 0u) return fail("mask past the end", nwords, n, 0);
        for (int v = 0; v < windows; ++v, ++cases) {
            uint64_t first, count;
            switch (v % 8) {
            case 0: first = 0, count = k; break;                                     // everything
            case 1: first = k + rng() % 3, count = 1 + rng() % 50; break;            // first >= k
            case 2: first = rng() % (k + 1), count = 0; break;                       // empty window
            case 3: first = rng() % (k + 1), count = ~0ull - (rng() % 2); break;     // "to the end"
            case 4: first = 32 * (rng() % (k / 32 + 1)), count = 32 * (1 + rng() % 9); break;    // on multiples of 32
            case 5: first = 256 * (rng() % (k / 256 + 1)), count = 256 * (1 + rng() % 3); break;  // ... of 256
            default: first = rng() % (k + 2), count = 1 + rng() % (k + 2); break;    // cutting words and chunks
            }
            const uint64_t want = first < k ? (count < k - first ? count : k - first) : 0;
            written.assign(want, 0u);
            // the plain loop: rank r of point u; the window owns r iff first <= r < first + count
            uint64_t cur_chunk = ~0ull;
            bool cur_skip = false;
            for (uint64_t r = 0; r < k; ++r) {
                const uint64_t u = ranked[r], c = u / 256;
                if (c != cur_chunk) {
                    const uint64_t lo = scan[8 * c], hi = 8 * c + 8 < nwords ? scan[8 * c + 8] : k;
                    cur_skip = rtr::extract_chunk_skip(lo, hi, first, count);
                    cur_chunk = c;
                }
                const bool in = r >= first && r - first < count;
                uint64_t slot = ~0ull;
                const uint64_t rank = rtr::remove_rank(scan[u / 32], words[u / 32], (uint32_t)u);
                if (rank != r) return fail("rank", u, rank, r);
                if (rtr::extract_slot(rank, first, count, &slot) != in) return fail("slot decision", u, first, count);
                if (!in) continue;
                if (cur_skip) return fail("skipped a chunk that owns a rank of the window", c, first, count);
                if (slot != r - first || slot >= want) return fail("slot", u, slot, r - first);
                ++written[slot];
                ++placed;
            }
            for (uint64_t j = 0; j < want; ++j)
                if (written[j] != 1u) return fail("slot coverage", j, written[j], want);
            // every chunk: the decision counted; an empty chunk or an empty window is always skipped
            for (uint64_t c = 0; c < nch; ++c) {
                const uint64_t lo = scan[8 * c], hi = 8 * c + 8 < nwords ? scan[8 * c + 8] : k;
                const bool skip = rtr::extract_chunk_skip(lo, hi, first, count);
                const bool owns = hi > lo && want > 0 && hi > first && lo < first + want;
                if (skip != !owns) return fail("chunk decision", c, first, count);  // (the rejection is exact, not only safe)
                skip ? ++skipped : ++kept_chunks;
            }
            // every point, resident order: the chunks of the window
            if (v % 4 == 0) {
                const uint64_t f = rng() % n, cnt = 1 + rng() % (n - f);
                uint64_t c0 = 0, c1 = 0;
                rtr::extract_all_chunks(f, cnt, &c0, &c1);
                if (c0 != f / 256 || c1 != (f + cnt - 1) / 256 + 1 || c1 > nch || c0 >= c1) return fail("all chunks", f, cnt, c1);
            }
        }
    }
    printf("ok %llu %llu %llu %llu\n", cases, skipped, kept_chunks, placed);
    return 0;
}
