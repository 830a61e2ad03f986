// Host-side check of rtr::chunk_box (csrc/rtr_chunk_box.h) against decoded values: for random chunks of 256 fp32
// bit patterns it builds the header word the packer writes (common prefix, widths, wide flag), decodes every value
// as base | low bits and asserts that each lies inside the box the helper returns, that the box's ends are values of
// the chunk's prefix, and that a wide chunk or one whose box reaches exponent 0xFF has no box.  Prints "ok <n>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "rtr_chunk_box.h"

static float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

int main() {
    std::mt19937_64 rng(0xC0FFEE05u);
    const uint32_t specials[] = {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x7F7FFFFFu, 0xFF7FFFFFu,
                                 0x00000001u, 0x807FFFFFu, 0x3F800000u, 0xBF800000u};
    long checked = 0, boxes = 0;
    for (int t = 0; t < 20000; ++t) {
        uint32_t v[3][256], base[3], w[3];
        for (int a = 0; a < 3; ++a) {
            const int mode = (int)(rng() % 6);
            const uint32_t b = (uint32_t)(rng() % 27);  // spread of the random low bits (26: wider than the packer's 25)
            uint32_t centre = (uint32_t)rng();
            if (mode == 0) centre = specials[rng() % (sizeof(specials) / sizeof(specials[0]))];
            if (mode == 1) centre = 0x7F000000u | (centre & 0x00FFFFFFu);  // near FLT_MAX: the box may reach 0xFF
            if (mode == 2) centre &= 0x80FFFFFFu;                           // denormals and tiny values
            for (int i = 0; i < 256; ++i) {
                uint32_t x = b ? ((centre & ~((1u << b) - 1u)) | ((uint32_t)rng() & ((1u << b) - 1u))) : centre;
                if (mode == 3 && (rng() % 64) == 0) x = specials[rng() % (sizeof(specials) / sizeof(specials[0]))];
                if (mode == 4 && i >= 200) x = v[a][199];  // a partial last chunk: copies of its last value
                v[a][i] = x;
            }
            uint32_t diff = 0;
            for (int i = 0; i < 256; ++i) diff |= v[a][i] ^ v[a][0];
            const uint32_t nb = diff ? 32u - (uint32_t)__builtin_clz(diff) : 0u;
            w[a] = nb > 25u ? 32u : nb;  // (k_pack_header)
            base[a] = w[a] == 32u ? 0u : (v[a][0] >> w[a]) << w[a];
        }
        const uint32_t wide = (w[0] == 32u || w[1] == 32u || w[2] == 32u) ? rtr::kPackWideFlag : 0u;
        const uint32_t widths = w[0] | (w[1] << 6) | (w[2] << 12) | wide;
        float lo[3], hi[3];
        const bool ok = rtr::chunk_box(base[0], base[1], base[2], widths, lo, hi);
        bool reaches_ff = false;
        for (int a = 0; a < 3; ++a)
            if (w[a] < 32u && ((base[a] | ((1u << w[a]) - 1u)) & 0x7F800000u) == 0x7F800000u) reaches_ff = true;
        if (ok != (!wide && !reaches_ff)) { std::printf("FAIL box presence, chunk %d\n", t); return 1; }
        if (!ok) continue;
        ++boxes;
        for (int a = 0; a < 3; ++a) {
            if (!(lo[a] <= hi[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a])) { std::printf("FAIL box ends, chunk %d\n", t); return 1; }
            for (int i = 0; i < 256; ++i) {
                const uint32_t dec = base[a] | (v[a][i] & ((1u << w[a]) - 1u));  // what the kernel decodes
                const float f = as_float(dec);
                if (dec != v[a][i] || !(f >= lo[a] && f <= hi[a])) {
                    std::printf("FAIL chunk %d axis %d value %d: %08x not in [%a, %a]\n", t, a, i, dec, lo[a], hi[a]);
                    return 1;
                }
                ++checked;
            }
        }
    }
    std::printf("ok %ld %ld\n", boxes, checked);
    return 0;
}
