// The tile store's frame-stamp rule (csrc/rtr_stamp_rule.h) built with plain g++ and walked through its wrap.
//
// Model of what the rule protects: `live[s]` = a directory word carrying stamp s may still be in the store.  A store
// whose stamp is c (by its frames, or by option "debug_store_stamp", which only moves forward) may hold words of every
// stamp 1 .. c, so the walk from c starts with all of those live.  Every step takes the next stamp; a requested clear
// empties `live` first.  The rule is right when no step ever takes stamp 0, a stamp above 24 bits or a live stamp --
// i.e. the clear comes before the first reuse of any value -- and when it asks for no clear it does not need: the
// 2^24 - 1 non-zero stamps are each used exactly once between two clears, so consecutive clears are exactly 2^24 - 1
// steps apart, and the first one comes when the walk leaves 0xFFFFFF.
// Then the size of the clear: kDirK 8-byte words per 32x16 storage tile, for five resolutions.
// Prints "ok <checks>".
#include <algorithm>
#include <cstdio>
#include <vector>

#include "rtr_stamp_rule.h"

static long long checks = 0;
#define CHECK(cond)                                             \
    do {                                                        \
        ++checks;                                               \
        if (!(cond)) {                                          \
            printf("FAIL line %d: %s\n", __LINE__, #cond);      \
            return 1;                                           \
        }                                                       \
    } while (0)

static int walk(uint32_t start, long long steps) {
    const uint32_t kValues = 1u << 24;
    std::vector<unsigned char> live(kValues, 0);
    for (uint32_t s = 1; s <= start; ++s) live[s] = 1;
    uint32_t cur = start;
    long long last_clear = -1, clears = 0;
    for (long long k = 1; k <= steps; ++k) {
        const rtr::StampStep st = rtr::next_stamp(cur);
        if (st.clear) {
            // the first clear: when the walk leaves 0xFFFFFF; every later one: 2^24 - 1 steps after the last
            if (last_clear < 0) CHECK(k == (long long)(0xFFFFFFu - start) + 1);
            else CHECK(k - last_clear == (long long)kValues - 1);
            CHECK(cur == 0xFFFFFFu && st.stamp == 1u);
            std::fill(live.begin(), live.end(), 0);
            last_clear = k;
            ++clears;
        }
        if (st.stamp == 0u || st.stamp > rtr::kStampMask || live[st.stamp]) {
            printf("FAIL start %u step %lld: stamp %u (live %d)\n", start, k, st.stamp, st.stamp < kValues ? live[st.stamp] : -1);
            return 1;
        }
        ++checks;
        if (!st.clear) CHECK(st.stamp == cur + 1u);  // (no clear: simply the next value)
        live[st.stamp] = 1;
        cur = st.stamp;
    }
    // as many clears as the walk's length allows, no fewer
    const long long first = (long long)(0xFFFFFFu - start) + 1;
    CHECK(clears == (steps < first ? 0 : 1 + (steps - first) / ((long long)kValues - 1)));
    return 0;
}

int main() {
    CHECK(rtr::kStampMask == 0xFFFFFFu);
    // a new store (0), a young one, the middle, a few frames short of the wrap (what the GPU tests set), the last value
    const uint32_t starts[] = {0u, 1u, 2u, 0x7FFFFFu, 0xFFFFF0u, 0xFFFFFDu, 0xFFFFFEu, 0xFFFFFFu};
    for (uint32_t s : starts)
        if (walk(s, (2ll << 24) + 100)) return 1;  // two full rounds: the first wrap and the one after it
    // the steps next to the wrap, spelled out
    CHECK(rtr::next_stamp(0u).stamp == 1u && !rtr::next_stamp(0u).clear);
    CHECK(rtr::next_stamp(0xFFFFFDu).stamp == 0xFFFFFEu && !rtr::next_stamp(0xFFFFFDu).clear);
    CHECK(rtr::next_stamp(0xFFFFFEu).stamp == 0xFFFFFFu && !rtr::next_stamp(0xFFFFFEu).clear);
    CHECK(rtr::next_stamp(0xFFFFFFu).stamp == 1u && rtr::next_stamp(0xFFFFFFu).clear);
    // bytes to clear = nst * kDirK * 8, nst = ceil(W / 32) * ceil(H / 16) storage tiles
    CHECK(rtr::kDirK == 21);
    const struct { int W, H, nst; size_t bytes; } res[] = {{16, 16, 1, 168}, {64, 48, 6, 1008}, {160, 128, 40, 6720},
                                                          {1920, 1080, 4080, 685440}, {3840, 2160, 16200, 2721600}};
    for (const auto &r : res) {
        const int nst = ((r.W + 31) / 32) * ((r.H + 15) / 16);
        CHECK(nst == r.nst);
        CHECK(rtr::dir_bytes(nst) == (size_t)nst * rtr::kDirK * 8);
        CHECK(rtr::dir_bytes(nst) == r.bytes);
    }
    printf("ok %lld\n", checks);
    return 0;
}
