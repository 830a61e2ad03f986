// The host arithmetic of rtr_fit_plane (csrc/rtr_plane_fit.h, rtr.h section 6j) built with plain g++ -ffp-contract=off
// -fno-fast-math, for tests/test_cpp_planes.py to compare bit for bit with tests/planes_ref.py.
//   plane_fit_check <in.bin> <out.bin>
// in:  u64 seed, u64 draws, f32 dist, u64 count, then per triple 9 x f32 (p0, p1, p2) and 3 x u64 ranks (60 bytes).
// out: `draws` x u64 (the sampler's first draws), then per triple u32 ok, 4 x f32 plane, 5 x f32 band (40 bytes; zeros
//      behind ok = 0).  Prints "ok <count> <non-degenerate>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rtr_plane_fit.h"

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: plane_fit_check in.bin out.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    uint64_t seed = 0, draws = 0, count = 0;
    float dist = 0.f;
    if (!f || fread(&seed, 8, 1, f) != 1 || fread(&draws, 8, 1, f) != 1 || fread(&dist, 4, 1, f) != 1 || fread(&count, 8, 1, f) != 1) return 2;
    std::vector<unsigned char> in((size_t)count * 60);
    if (count && fread(in.data(), 60, count, f) != count) return 2;
    fclose(f);
    std::vector<uint64_t> z(draws);
    for (uint64_t t = 0; t < draws; ++t) z[t] = rtr::plane_draw(seed, t);
    std::vector<unsigned char> out((size_t)count * 40, 0);
    uint64_t good = 0;
    for (uint64_t i = 0; i < count; ++i) {
        float p[9], rec[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        uint64_t r[3];
        memcpy(p, in.data() + 60 * i, 36);
        memcpy(r, in.data() + 60 * i + 36, 24);
        const uint32_t ok = rtr::plane_candidate(p, p + 3, p + 6, r, rec) ? 1u : 0u;
        if (ok) rtr::plane_band(rec, dist, rec + 4), ++good;
        else memset(rec, 0, sizeof rec);
        memcpy(out.data() + 40 * i, &ok, 4);
        memcpy(out.data() + 40 * i + 4, rec, 36);
    }
    f = fopen(argv[2], "wb");
    if (!f || (draws && fwrite(z.data(), 8, draws, f) != draws) || (count && fwrite(out.data(), 40, count, f) != count)) return 2;
    fclose(f);
    printf("ok %llu %llu\n", (unsigned long long)count, (unsigned long long)good);
    return 0;
}
