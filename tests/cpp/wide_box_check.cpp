// Host-side check of the wide chunks' box word (csrc/rtr_chunk_box.h: wide_box_word and the seven-argument chunk_box).
// The packer's header rule is restated here (pack_header: common prefix, widths, wide flag, and the word from the min /
// max of the first wide axis over the values below n); then
//   1. random chunks of bit patterns -- mixed signs, +-0, denormals, huge values, NaN / inf, one, two and three wide axes,
//      partial chunks whose tail is NaN padding: every value below n lies inside the box, the word's ends are within 2^-7
//      of the exact ones, there is no box exactly for a non-finite value below n, a rounded end of exponent 0xFF or a
//      prefix axis that reaches it, further wide axes are [-FLT_MAX, FLT_MAX], the six-argument chunk_box is what it was
//      and the seven-argument one equals it on chunks that are not wide, and no clip plane set rejects (clip_box_outside)
//      a box holding a point clip_keep keeps;
//   2. chunks of a room-sized scene that straddle one, two or three coordinate planes under random cameras: box_outside
//      never rejects a box holding a point the oracle's projection puts on a pixel (orc_project_point), and it does
//      reject a good share of the others.
// With two arguments it only encodes: pairs of patterns (min, max) read from the first file, their words written to the
// second (tests/test_wide_box.py compares them with a numpy restatement).
// Prints "ok <wide> <boxed> <values> <clip rejected> <scene chunks> <scene rejected> <scene in-frustum chunks>".
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "rtr_chunk_box.h"

extern "C" int64_t orc_project_point(const float P[16], float x, float y, float z, int W, int H, uint32_t* depth_bits);

static float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t as_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static bool finite_bits(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }

struct Header {
    uint32_t base[3], w[3], widths, wbox;
    int first_wide;
    bool all_finite;
    float vmin, vmax;  // of the first wide axis, over the values below n (when all are finite)
};
// what k_pack_measure writes for 256 patterns per axis of which the first nvalid are points (the rest: padding)
static Header pack_header(const uint32_t v[3][256], int nvalid) {
    Header h{};
    h.first_wide = -1;
    for (int a = 0; a < 3; ++a) {
        uint32_t diff = 0;
        for (int i = 0; i < 256; ++i) diff |= v[a][i] ^ v[a][0];
        const uint32_t nb = diff ? 32u - (uint32_t)__builtin_clz(diff) : 0u;
        h.w[a] = nb > 25u ? 32u : nb;
        h.base[a] = h.w[a] == 32u ? 0u : (v[a][0] >> h.w[a]) << h.w[a];
        if (h.w[a] == 32u && h.first_wide < 0) h.first_wide = a;
    }
    h.widths = h.w[0] | (h.w[1] << 6) | (h.w[2] << 12) | (h.first_wide >= 0 ? rtr::kPackWideFlag : 0u);
    h.all_finite = true;
    for (int a = 0; a < 3; ++a)
        for (int i = 0; i < nvalid; ++i) h.all_finite = h.all_finite && finite_bits(v[a][i]);
    if (h.first_wide >= 0 && h.all_finite) {
        uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
        for (int i = 0; i < nvalid; ++i) {
            const uint32_t k = rtr::float_order_key(v[h.first_wide][i]);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
        h.vmin = as_float(rtr::float_order_bits(kmin)), h.vmax = as_float(rtr::float_order_bits(kmax));
        h.wbox = rtr::wide_box_word(rtr::float_order_bits(kmin), rtr::float_order_bits(kmax));
    }
    return h;
}

int main(int argc, char **argv) {
    if (argc == 3) {  // the encoding alone: pairs of patterns (min, max) from argv[1], their words to argv[2]
        std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
        if (!in || !out) return 2;
        uint32_t pr[2];
        while (std::fread(pr, 4, 2, in) == 2) {
            const uint32_t w = rtr::wide_box_word(pr[0], pr[1]);
            std::fwrite(&w, 4, 1, out);
        }
        std::fclose(in);
        std::fclose(out);
        return 0;
    }
    std::mt19937_64 rng(0xB0C5ull);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    const uint32_t zeros[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu};
    const uint32_t huge[] = {0x7F7FFFFFu, 0xFF7FFFFFu, 0x7F7F0000u, 0xFF7F0000u, 0x7F7F0001u, 0xFF7F0001u, 0x7F000000u, 0xFE800000u};
    const uint32_t bad[] = {0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00001u};
    // the keys order the finite patterns as the floats compare (+-0 apart)
    for (int t = 0; t < 200000; ++t) {
        uint32_t a = (uint32_t)rng(), b = (uint32_t)rng();
        if (!finite_bits(a) || !finite_bits(b)) continue;
        if (rtr::float_order_bits(rtr::float_order_key(a)) != a) { std::printf("FAIL key round trip %08x\n", a); return 1; }
        if ((as_float(a) < as_float(b)) && !(rtr::float_order_key(a) < rtr::float_order_key(b))) { std::printf("FAIL key order %08x %08x\n", a, b); return 1; }
    }
    if (!(rtr::float_order_key(0x80000000u) < rtr::float_order_key(0u))) { std::printf("FAIL key order of -0, +0\n"); return 1; }

    long wide_chunks = 0, boxed = 0, values = 0, clip_rej = 0, by_axes[4] = {0, 0, 0, 0};
    for (int t = 0; t < 60000; ++t) {
        uint32_t v[3][256];
        const int want_wide = (int)(rng() % 4);  // axes forced wide (others may turn out wide by themselves)
        const int nvalid = (rng() % 4 == 0) ? 1 + (int)(rng() % 256) : 256;
        const int poison = (int)(rng() % 6);  // 0: a NaN / inf somewhere below n, 1: one in the padding only
        for (int a = 0; a < 3; ++a) {
            const int mode = a < want_wide ? (int)(rng() % 5) : 5 + (int)(rng() % 2);
            const uint32_t nb = (uint32_t)(rng() % 26), centre = ((uint32_t)rng() & 0x7FFFFFFFu) % 0x7F000000u;
            for (int i = 0; i < 256; ++i) {
                uint32_t x = (centre & ~((1u << nb) - 1u)) | ((uint32_t)rng() & ((1u << nb) - 1u));  // a prefix axis ...
                if (mode == 0) x ^= (uint32_t)(rng() & 1) << 31;                                    // ... with mixed signs
                if (mode == 1) x = zeros[rng() % 6] ^ ((rng() % 4 == 0) ? ((uint32_t)rng() & 0x3FFu) : 0u);  // +-0, denormals
                if (mode == 2) x = huge[rng() % 8];                                                 // the largest magnitudes
                if (mode == 3) x = (uint32_t)rng() % 0x7F800000u | ((uint32_t)(rng() & 1) << 31);   // anything finite
                if (mode == 4) x = as_bits((float)(0.05 * (u01(rng) - 0.4)));                       // a wall next to a plane
                if (mode == 6) x = centre;                                                          // constant
                if (a == 2 && mode >= 5 && (rng() % 3 == 0)) x |= 0x80000000u;
                v[a][i] = x;
            }
            if (mode >= 5 && (rng() & 1))  // (a prefix axis of one sign)
                for (int i = 0; i < 256; ++i) v[a][i] = (v[a][i] & 0x7FFFFFFFu) | (v[a][0] & 0x80000000u);
        }
        if (poison == 0) v[rng() % 3][rng() % nvalid] = bad[rng() % 4];
        for (int i = nvalid; i < 256; ++i)  // the tail: copies of the last point, or (the cloud's last quad) NaN padding
            for (int a = 0; a < 3; ++a) v[a][i] = (poison == 1 && i < ((nvalid + 3) & ~3)) ? 0x7FC00000u : v[a][nvalid - 1];
        const Header h = pack_header(v, nvalid);
        const bool wide = h.first_wide >= 0;
        int nwide = 0;
        bool prefix_ff = false;
        for (int a = 0; a < 3; ++a) {
            nwide += h.w[a] == 32u;
            if (h.w[a] < 32u && !finite_bits(h.base[a] | ((1u << h.w[a]) - 1u))) prefix_ff = true;
        }
        // the six-argument form: as before
        float lo6[3], hi6[3], lo[3], hi[3];
        const bool ok6 = rtr::chunk_box(h.base[0], h.base[1], h.base[2], h.widths, lo6, hi6);
        if (ok6 != (!wide && !prefix_ff)) { std::printf("FAIL six-argument presence, chunk %d\n", t); return 1; }
        if (!wide) {  // ... and the new form equals it whatever the word
            const bool ok7 = rtr::chunk_box(h.base[0], h.base[1], h.base[2], h.widths, (uint32_t)rng(), lo, hi);
            if (ok7 != ok6 || std::memcmp(lo, lo6, sizeof lo) != 0 || std::memcmp(hi, hi6, sizeof hi) != 0) { std::printf("FAIL seven != six, chunk %d\n", t); return 1; }
            if (h.wbox != 0u) { std::printf("FAIL word on a chunk that is not wide, chunk %d\n", t); return 1; }
            continue;
        }
        ++wide_chunks;
        if (rtr::chunk_box(h.base[0], h.base[1], h.base[2], h.widths, 0u, lo, hi)) { std::printf("FAIL word 0 gives a box, chunk %d\n", t); return 1; }
        // the word exists exactly for finite chunks whose rounded ends stay finite
        const bool end_ff = h.all_finite && (as_bits(h.vmin) > 0xFF7F0000u || (as_bits(h.vmax) > 0x7F7F0000u && as_bits(h.vmax) < 0x80000000u));
        if ((h.wbox != 0u) != (h.all_finite && !end_ff)) { std::printf("FAIL word presence, chunk %d (%08x)\n", t, h.wbox); return 1; }
        const bool ok = rtr::chunk_box(h.base[0], h.base[1], h.base[2], h.widths, h.wbox, lo, hi);
        if (ok != (h.wbox != 0u && !prefix_ff)) { std::printf("FAIL box presence, chunk %d\n", t); return 1; }
        if (!ok) continue;
        ++boxed, ++by_axes[nwide];
        for (int a = 0; a < 3; ++a) {
            if (!(lo[a] <= hi[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a])) { std::printf("FAIL box ends, chunk %d\n", t); return 1; }
            if (h.w[a] == 32u && a != h.first_wide && (lo[a] != -FLT_MAX || hi[a] != FLT_MAX)) { std::printf("FAIL unbounded axis, chunk %d\n", t); return 1; }
            if (h.w[a] < 32u && (lo[a] != lo6[a] || hi[a] != hi6[a])) { std::printf("FAIL prefix axis changed, chunk %d\n", t); return 1; }
            for (int i = 0; i < nvalid; ++i) {
                const float f = as_float(v[a][i]);
                if (!(f >= lo[a] && f <= hi[a])) { std::printf("FAIL chunk %d axis %d value %d: %a not in [%a, %a]\n", t, a, i, f, lo[a], hi[a]); return 1; }
                ++values;
            }
        }
        {  // tightness of the word's ends: within 2^-7 of the exact end's magnitude (+ one denormal step of the format)
            const int a = h.first_wide;
            const double slack_lo = std::fabs((double)h.vmin) * 0x1p-7 + 0x1p-133, slack_hi = std::fabs((double)h.vmax) * 0x1p-7 + 0x1p-133;
            if ((double)lo[a] < (double)h.vmin - slack_lo || (double)hi[a] > (double)h.vmax + slack_hi) { std::printf("FAIL loose ends, chunk %d\n", t); return 1; }
        }
        // clip planes: a rejected box holds no kept point
        for (int r = 0; r < 4; ++r) {
            rtr::Clip c{};
            c.count = 1 + (int)(rng() % 3);
            for (int j = 0; j < c.count; ++j) {
                const int i = (int)(rng() % nvalid);  // a plane near one of the chunk's points
                double d = 0;
                for (int k = 0; k < 3; ++k) {
                    c.p[j][k] = (rng() % 3 == 0) ? 0.f : (float)(2.0 * u01(rng) - 1.0);
                    d -= (double)c.p[j][k] * (double)as_float(v[k][i]);
                }
                c.p[j][3] = (float)(d * (1.0 + 0.5 * (u01(rng) - 0.5)) + (rng() % 2 ? 0.0 : 1e-3 * (u01(rng) - 0.5)));
                if (!std::isfinite(c.p[j][3])) c.p[j][3] = 0.f;
            }
            if (!rtr::clip_box_outside(c, lo, hi)) continue;
            ++clip_rej;
            for (int i = 0; i < nvalid; ++i)
                if (rtr::clip_keep(c, as_float(v[0][i]), as_float(v[1][i]), as_float(v[2][i]))) { std::printf("FAIL chunk %d: rejected by the clip planes, point %d kept\n", t, i); return 1; }
        }
    }
    if (by_axes[1] < 1000 || by_axes[2] < 1000 || by_axes[3] < 1000) { std::printf("FAIL coverage %ld %ld %ld\n", by_axes[1], by_axes[2], by_axes[3]); return 1; }

    // 2. a room around the origin: chunks on the coordinate planes against random cameras
    long scene = 0, scene_rej = 0, scene_in = 0;
    for (int t = 0; t < 40000; ++t) {
        const int W = (rng() & 1) ? 64 : 1920, H = W == 64 ? 48 : 1080;
        const double f = 0.8 * W, ay = 6.2831853 * u01(rng), ax = 0.6 * (u01(rng) - 0.5);
        const double R[3][3] = {{std::cos(ay), 0, std::sin(ay)},
                                {std::sin(ax) * std::sin(ay), std::cos(ax), -std::sin(ax) * std::cos(ay)},
                                {-std::cos(ax) * std::sin(ay), std::sin(ax), std::cos(ax) * std::cos(ay)}};
        double cpos[3] = {6 * (u01(rng) - 0.5), 3 * (u01(rng) - 0.5), 6 * (u01(rng) - 0.5)};
        if (rng() % 4 == 0) cpos[rng() % 3] = 0.0;  // a camera sitting on a coordinate plane
        float P[16] = {0};
        for (int j = 0; j < 3; ++j) {
            P[j] = (float)(f * R[0][j] + 0.5 * W * R[2][j]);
            P[4 + j] = (float)(f * R[1][j] + 0.5 * H * R[2][j]);
            P[8 + j] = (float)R[2][j];
        }
        const double t0 = -(R[0][0] * cpos[0] + R[0][1] * cpos[1] + R[0][2] * cpos[2]);
        const double t1 = -(R[1][0] * cpos[0] + R[1][1] * cpos[1] + R[1][2] * cpos[2]);
        const double t2 = -(R[2][0] * cpos[0] + R[2][1] * cpos[1] + R[2][2] * cpos[2]);
        P[3] = (float)(f * t0 + 0.5 * W * t2), P[7] = (float)(f * t1 + 0.5 * H * t2), P[11] = (float)t2, P[15] = 1.f;
        const rtr::FrustumPlanes fp = rtr::frustum_planes(P, (float)W, (float)H);
        for (int b = 0; b < 4; ++b) {
            uint32_t v[3][256];
            const int straddle = 1 + (int)(rng() % 3);
            const double size = std::pow(10.0, -2.5 + 2.5 * u01(rng));
            for (int a = 0; a < 3; ++a) {
                const double c0 = a < straddle ? size * (u01(rng) - 0.5) * 0.9 : 10.0 * (u01(rng) - 0.5);
                for (int i = 0; i < 256; ++i) v[a][i] = as_bits((float)(c0 + size * (u01(rng) - 0.5)));
            }
            const Header h = pack_header(v, 256);
            float lo[3], hi[3];
            if (h.first_wide < 0 || !rtr::chunk_box(h.base[0], h.base[1], h.base[2], h.widths, h.wbox, lo, hi)) continue;
            ++scene;
            bool in = false;
            for (int i = 0; i < 256 && !in; ++i) in = orc_project_point(P, as_float(v[0][i]), as_float(v[1][i]), as_float(v[2][i]), W, H, nullptr) >= 0;
            const bool rej = rtr::box_outside(fp, lo, hi);
            scene_in += in, scene_rej += rej;
            if (rej && in) { std::printf("FAIL scene %d: a box with an in-frustum point rejected\n", t); return 1; }
        }
    }
    std::printf("ok %ld %ld %ld %ld %ld %ld %ld\n", wide_chunks, boxed, values, clip_rej, scene, scene_rej, scene_in);
    return 0;
}
