// estimateNormals of include/rtr_project_cloud.hpp (rtr_normals.h section 6o) over the C ABI, built with plain g++.  The
// stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   normals_facade_check <cloud.bin> <params: radius as 1 float, k as 1 u32, the viewpoint as 3 floats .bin> <out_prefix>
// The program calls estimateNormals(k, radius, normals, curvature, found) and then, with the viewpoint,
// estimateNormals(k, radius, normals2, curvature2, nullptr, viewpoint); it writes <out>.normals / .curvature / .found,
// <out>.normals2 / .curvature2 and the two return values with selectedCount() before and after to <out>.counts
// (4 x u64).  Exit 8: the call created a selection.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "rtr_project_cloud.hpp"

struct P3 { float x, y, z; };
struct C3 { unsigned char v[3]; unsigned char operator[](int i) const { return v[i]; } };
struct Block { std::vector<P3> positions; std::vector<C3> colors; };

static void dump(const std::string& path, const void* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { perror(path.c_str()); exit(2); }
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    unsigned long long n = 0;
    if (!f || fread(&n, 8, 1, f) != 1) return 2;
    std::vector<P3> pts(n); std::vector<C3> cols(n);
    if (fread(pts.data(), 12, n, f) != n || fread(cols.data(), 3, n, f) != n) return 2;
    fclose(f);
    float r, view[3]; uint32_t k;
    f = fopen(argv[2], "rb");
    if (!f || fread(&r, 4, 1, f) != 1 || fread(&k, 4, 1, f) != 1 || fread(view, 4, 3, f) != 3) return 2;
    fclose(f);
    const std::string out = argv[3];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        std::vector<float> normals(n * 3, 7.f), curvature(n, 7.f), normals2(n * 3, 7.f), curvature2(n, 7.f);
        std::vector<uint32_t> found(n, 7u);
        uint64_t counts[4];
        counts[2] = pc.selectedCount();
        counts[0] = pc.estimateNormals(k, r, normals.data(), curvature.data(), found.data());
        counts[1] = pc.estimateNormals(k, r, normals2.data(), curvature2.data(), nullptr, view);
        counts[3] = pc.selectedCount();
        int set = 1;
        if (rtr_get_option(pc.context(), "selection", &set) != RTR_OK || set != 0) return 8;
        static_assert(RTR_NORMAL_MAX_K == 64 && RTR_NORMAL_MIN_FOUND == 2 && RTR_NORMAL_VIEWPOINT == 1, "rtr_normals.h through the facade");
        dump(out + ".normals", normals.data(), n * 12);
        dump(out + ".curvature", curvature.data(), n * 4);
        dump(out + ".found", found.data(), n * 4);
        dump(out + ".normals2", normals2.data(), n * 12);
        dump(out + ".curvature2", curvature2.data(), n * 4);
        dump(out + ".counts", counts, sizeof counts);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
