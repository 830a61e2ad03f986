// csrc/rtr_segment_rule.h -- the edge rule of rtr_select_segments (include/rtr_segments.h section 6q) as the kernels call
// it -- built with plain g++ (-ffp-contract=off -fno-fast-math) as a stand-alone program, plainly and with
// -fsanitize=address,undefined.
//   segment_rule_check <case.bin> [<case.bin> ...]
// A case, written by tests/test_cpp_segments.py from the numpy reference: u64 n; f32 r2, cos_angle, max_curvature; u32
// oriented, has_curvature; n x 3 f32 coordinates; n x 3 f32 normals; n f32 curvatures (when has_curvature); u64 e; e
// pairs of u32 (i, j), i < j, ascending: the reference's JOINED pairs.
// For every i < j the program forms the contract's relation -- both points finite, the distance test in the contract's
// order, segment_usable of both, segment_joined -- from EITHER end, and a second time the way the library does it:
// normals gathered with (+0, +0, +0) for a point that is not usable, then segment_joined alone.  All four must be the
// reference's edge list (exit 10: the rule differs; 11: not symmetric; 12: the gathered form differs).  Prints the
// pairs tested and the edges found.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "rtr_segment_rule.h"

static float dist2(const float* a, const float* b) {  // ((dx dx + dy dy) + dz dz), every operation rounded on its own
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
}

static bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

template <class T>
static void rd(FILE* f, T* p, size_t count) {
    if (count && fread(p, sizeof(T), count, f) != count) { fprintf(stderr, "short case file\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: segment_rule_check <case.bin> ...\n"); return 2; }
    unsigned long long tested = 0, found = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { perror(argv[a]); return 2; }
        uint64_t n = 0, e = 0;
        float par[3];
        uint32_t flag[2];
        rd(f, &n, 1); rd(f, par, 3); rd(f, flag, 2);
        std::vector<float> xyz(3 * n), nrm(3 * n), curv(flag[1] ? n : 0);
        rd(f, xyz.data(), xyz.size()); rd(f, nrm.data(), nrm.size()); rd(f, curv.data(), curv.size());
        rd(f, &e, 1);
        std::vector<uint32_t> want(2 * e);
        rd(f, want.data(), want.size());
        fclose(f);
        const float r2 = par[0], cos_angle = par[1], max_curvature = par[2];
        const bool oriented = flag[0] != 0;
        std::vector<char> ok(n, 1);
        std::vector<float> gat(nrm);
        for (uint64_t i = 0; i < n; ++i) {
            if (flag[1]) ok[i] = rtr::segment_usable(curv[i], max_curvature);
            if (!ok[i]) gat[3 * i] = gat[3 * i + 1] = gat[3 * i + 2] = 0.f;
        }
        std::vector<std::pair<uint32_t, uint32_t>> got;
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t j = i + 1; j < n; ++j) {
                const float *p = &xyz[3 * i], *q = &xyz[3 * j], *u = &nrm[3 * i], *v = &nrm[3 * j], *gu = &gat[3 * i], *gv = &gat[3 * j];
                const bool near = finite3(p) && finite3(q) && dist2(p, q) <= r2, near_back = finite3(p) && finite3(q) && dist2(q, p) <= r2;
                const bool fwd = near && ok[i] && ok[j] && rtr::segment_joined(u[0], u[1], u[2], v[0], v[1], v[2], cos_angle, oriented);
                const bool back = near_back && ok[j] && ok[i] && rtr::segment_joined(v[0], v[1], v[2], u[0], u[1], u[2], cos_angle, oriented);
                const bool lib = near && rtr::segment_joined(gu[0], gu[1], gu[2], gv[0], gv[1], gv[2], cos_angle, oriented);
                const bool lib_back = near_back && rtr::segment_joined(gv[0], gv[1], gv[2], gu[0], gu[1], gu[2], cos_angle, oriented);
                ++tested;
                if (fwd != back || lib != lib_back) { fprintf(stderr, "%s: pair %llu %llu is not symmetric\n", argv[a], (unsigned long long)i, (unsigned long long)j); return 11; }
                if (fwd != lib) { fprintf(stderr, "%s: pair %llu %llu: the gathered form differs\n", argv[a], (unsigned long long)i, (unsigned long long)j); return 12; }
                if (fwd) got.emplace_back((uint32_t)i, (uint32_t)j);
            }
        bool same = got.size() == e;
        for (size_t k = 0; same && k < got.size(); ++k) same = got[k].first == want[2 * k] && got[k].second == want[2 * k + 1];
        if (!same) { fprintf(stderr, "%s: %zu edges, the reference has %llu\n", argv[a], got.size(), (unsigned long long)e); return 10; }
        found += got.size();
    }
    printf("%llu pairs tested, %llu edges, %d cases\n", tested, found, argc - 1);
    return 0;
}
