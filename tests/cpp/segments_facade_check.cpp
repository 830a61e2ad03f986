// selectSegments / removeSmallSegments of include/rtr_project_cloud.hpp (rtr_segments.h section 6q) over the C ABI, built
// with plain g++.  The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   segments_facade_check <cloud.bin> <params: radius, angle, max_curvature as 3 floats, k, min as 2 u32 .bin> <want_prefix> <out_prefix>
// <want>.words0 and .words1 hold the words the reference expects after: selectSegments(radius, k, angle, max_curvature,
// min) with labels; selectSegments(radius, k, angle, INFINITY, 2, 49, false, ADD, outside).  <want>.labels holds the
// labels of the first step.  The program compares the selection after each step with them (exit 10 + step on a
// difference) and the labels the first step wrote (exit 9), writes the two counts, selectedCount(), the number
// removeSmallSegments(radius, k, angle, max_curvature, min) removed and the points left to <out>.counts (5 x u64) and the
// coordinates left, extracted, to <out>.xyz.  Exit 8: the selection was not gone after removeSmallSegments.
#include <cmath>
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
    if (argc < 5) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    unsigned long long n = 0;
    if (!f || fread(&n, 8, 1, f) != 1) return 2;
    std::vector<P3> pts(n); std::vector<C3> cols(n);
    if (fread(pts.data(), 12, n, f) != n || fread(cols.data(), 3, n, f) != n) return 2;
    fclose(f);
    float r[3]; uint32_t k[2];
    f = fopen(argv[2], "rb");
    if (!f || fread(r, 4, 3, f) != 3 || fread(k, 4, 2, f) != 2) return 2;
    fclose(f);
    const std::string want = argv[3], out = argv[4];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        std::vector<uint32_t> words((size_t)((n + 31) / 32)), ref(words.size());
        auto same_as = [&](const char* ext) {
            if (rtr_download_buffer(pc.context(), RTR_BUF_SELECTION, words.data(), words.size() * 4) != RTR_OK) exit(4);
            FILE* g = fopen((want + ext).c_str(), "rb");
            if (!g || fread(ref.data(), 4, ref.size(), g) != ref.size()) exit(2);
            fclose(g);
            return memcmp(words.data(), ref.data(), words.size() * 4) == 0;
        };
        uint64_t counts[5];
        std::vector<uint32_t> labels(n, 0xFFFFFFFFu), ref_labels(n);
        counts[0] = pc.selectSegments(r[0], k[0], r[1], r[2], k[1], 0, false, RTR_SELECT_REPLACE, false, labels.data());
        if (!same_as(".words0")) return 10;
        FILE* g = fopen((want + ".labels").c_str(), "rb");
        if (!g || fread(ref_labels.data(), 4, n, g) != n) return 2;
        fclose(g);
        if (memcmp(labels.data(), ref_labels.data(), n * 4) != 0) return 9;
        counts[1] = pc.selectSegments(r[0], k[0], r[1], INFINITY, 2, 49, false, RTR_SELECT_ADD, true);
        if (!same_as(".words1")) return 11;
        counts[2] = pc.selectedCount();
        counts[3] = pc.removeSmallSegments(r[0], k[0], r[1], r[2], k[1]);
        int set = 1;
        if (rtr_get_option(pc.context(), "selection", &set) != RTR_OK || set != 0 || pc.selectedCount() != 0) return 8;
        rtr_num_points(pc.context(), &counts[4]);
        dump(out + ".counts", counts, sizeof counts);
        std::vector<float> xyz; std::vector<uint8_t> rgb;
        pc.selectPlanes(nullptr, 0);  // (no plane: every vertex)
        pc.extractSelected(xyz, rgb);
        dump(out + ".xyz", xyz.data(), xyz.size() * 4);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
