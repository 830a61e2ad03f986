// The window arithmetic of rtr_write_points (csrc/rtr_write_index.h) built with plain g++ and fuzzed against a per-bit
// loop: for random words and scans, with first / count at 0, at k, at k +- 1 and at UINT64_MAX, n at every value from 1
// to 70 and at 2^32 - 1.  Over all words the window's bits must number min(count, k - first) and be contiguous in rank.
// Prints "ok <cases> <bits kept>".
#include <cstdio>
#include <random>
#include <vector>

#include "rtr_write_index.h"

static int fail(const char* what, unsigned long long a, unsigned long long b, unsigned long long c) {
    printf("FAIL %s %llu %llu %llu\n", what, a, b, c);
    return 1;
}

// the per-bit statement: bit b of word w survives iff its point lies below n and its rank r satisfies
// first <= r < first + count, the sum never formed
static uint32_t reference(uint32_t word, uint64_t scan, uint64_t w, uint64_t first, uint64_t count, uint64_t n) {
    uint32_t out = 0;
    uint64_t r = scan;
    for (uint32_t b = 0; b < 32; ++b) {
        if (w * 32 + b >= n || !((word >> b) & 1u)) continue;
        if (r >= first && r - first < count) out |= 1u << b;
        ++r;
    }
    return out;
}

static unsigned long long g_cases = 0, g_kept = 0;

// a whole selection of n points: every window, word by word against the reference, then count and contiguity
static int check_selection(const std::vector<uint32_t>& words, uint64_t n, std::mt19937_64& rng) {
    const uint64_t nwords = (n + 31) / 32;
    std::vector<uint32_t> scan(nwords);
    uint64_t k = 0;
    for (uint64_t w = 0; w < nwords; ++w) {
        scan[w] = (uint32_t)k;
        k += (uint64_t)__builtin_popcount(words[w] & rtr::extract_word_mask(w, n));
    }
    const uint64_t M = ~0ull;
    const uint64_t firsts[] = {0, 1, k ? k - 1 : 0, k, k + 1, k / 3, M, M - 1, rng() % (k + 2)};
    const uint64_t counts[] = {0, 1, k ? k - 1 : 0, k, k + 1, k / 2, M, M - 1, 5, 1 + rng() % (k + 2)};
    for (uint64_t first : firsts)
        for (uint64_t count : counts) {
            ++g_cases;
            const uint64_t want = first < k ? (count < k - first ? count : k - first) : 0;
            uint64_t got = 0, lo = M, hi = 0;  // the ranks of the kept bits
            for (uint64_t w = 0; w < nwords; ++w) {
                const uint32_t bits = rtr::write_word_bits(words[w], scan[w], w, first, count, n);
                if (bits != reference(words[w], scan[w], w, first, count, n)) return fail("word", w, first, count);
                if (bits & ~words[w]) return fail("bit outside the selection", w, bits, words[w]);
                if (bits & ~rtr::extract_word_mask(w, n)) return fail("bit at or past n", w, bits, n);
                for (uint32_t b = 0; b < 32; ++b) {
                    if (!((bits >> b) & 1u)) continue;
                    const uint64_t r = rtr::remove_rank(scan[w], words[w], b);
                    lo = r < lo ? r : lo, hi = r > hi ? r : hi;
                    ++got;
                }
            }
            if (got != want) return fail("count", got, want, first);
            if (got && (lo != first || hi - lo + 1 != got)) return fail("ranks not contiguous from first", lo, hi, got);
            g_kept += got;
        }
    return 0;
}

int main() {
    std::mt19937_64 rng(0x5EED0021ull);
    std::vector<uint32_t> words;
    // n at every value from 1 to 70: dense, sparse, all, none, random -- with garbage bits past n
    for (uint64_t n = 1; n <= 70; ++n)
        for (int t = 0; t < 60; ++t) {
            const uint64_t nwords = (n + 31) / 32;
            words.assign(nwords, 0u);
            for (auto& v : words) {
                v = (uint32_t)rng();
                if (t % 5 == 0) v |= (uint32_t)rng() | (uint32_t)rng();
                else if (t % 5 == 1) v &= (uint32_t)rng() & (uint32_t)rng();
                else if (t % 5 == 2) v = 0xFFFFFFFFu;
                else if (t % 5 == 3 && t % 2) v = 0u;
            }
            if (t % 3) words[nwords - 1] |= ~rtr::extract_word_mask(nwords - 1, n);
            if (int rc = check_selection(words, n, rng)) return rc;
        }
    // larger clouds whose windows cut words and chunks
    for (int t = 0; t < 300; ++t) {
        const uint64_t n = 71 + rng() % 3000, nwords = (n + 31) / 32;
        words.assign(nwords, 0u);
        for (auto& v : words) v = (uint32_t)rng() & (t % 2 ? (uint32_t)rng() : 0xFFFFFFFFu);
        if (int rc = check_selection(words, n, rng)) return rc;
    }
    // single words with arbitrary scans, n = 2^32 - 1 among them: the last word holds 31 points, the ranks reach 2^32 - 2
    const uint64_t big = 0xFFFFFFFFull, M = ~0ull;
    for (int t = 0; t < 400000; ++t, ++g_cases) {
        const uint64_t n = t % 2 ? big : 1 + rng() % big;
        const uint64_t w = t % 4 == 1 ? (n + 31) / 32 - 1 : rng() % ((n + 31) / 32 + 1);  // (one past the end too)
        uint32_t word = (uint32_t)rng();
        if (t % 7 == 0) word = 0xFFFFFFFFu;
        const uint32_t scan = t % 3 == 0 ? (uint32_t)(32 * w) : (uint32_t)(rng() % (32 * w + 1));  // (at most the points below)
        const uint64_t pc = (uint64_t)__builtin_popcount(word & rtr::extract_word_mask(w, n));
        uint64_t first, count;
        switch (t % 6) {
        case 0: first = scan, count = pc; break;
        case 1: first = scan + rng() % 33, count = rng() % 40; break;
        case 2: first = scan > 5 ? scan - rng() % 5 : 0, count = M - rng() % 2; break;
        case 3: first = M - rng() % 2, count = M; break;
        case 4: first = rng() % (scan + 34ull), count = 1 + rng() % 64; break;
        default: first = 0, count = scan + rng() % 33; break;
        }
        const uint32_t bits = rtr::write_word_bits(word, scan, w, first, count, n);
        if (bits != reference(word, scan, w, first, count, n)) return fail("single word", w, first, count);
        g_kept += (uint64_t)__builtin_popcount(bits);
    }
    // "every point": all-ones words with scan 32 w, the window [first, first + count) of the indices themselves
    for (int t = 0; t < 20000; ++t, ++g_cases) {
        const uint64_t n = t % 2 ? big : 1 + rng() % 100000, first = rng() % (n + 2), count = t % 5 ? rng() % (n + 2) : M;
        const uint64_t w = (first / 32 + rng() % 3) % ((n + 31) / 32);
        const uint32_t bits = rtr::write_word_bits(0xFFFFFFFFu, (uint32_t)(32 * w), w, first, count, n);
        uint32_t ref = 0;
        for (uint32_t b = 0; b < 32; ++b) {
            const uint64_t u = 32 * w + b;
            if (u < n && u >= first && u - first < count) ref |= 1u << b;
        }
        if (bits != ref) return fail("every point", w, first, count);
    }
    printf("ok %llu %llu\n", g_cases, g_kept);
    return 0;
}
