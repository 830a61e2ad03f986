// selectStatistical / removeStatisticalOutliers of include/rtr_project_cloud.hpp (rtr_statistics.h section 6n) over the C
// ABI, built with plain g++.  The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   statistical_facade_check <cloud.bin> <params: radius as 1 float, k as 1 u32, std_mul as 1 double .bin> <want_prefix> <out_prefix>
// <want>.words0 / .words1 hold the words the reference expects after: selectStatistical(k, radius, std_mul) with all three
// outputs; selectStatistical(k, radius, std_mul, TOGGLE, outside).  <want>.mean / .found hold the first call's arrays.
// The program compares the selection after each step (exit 10 + step on a difference) and the two arrays bit for bit
// (exit 20 / 21), writes the two counts, selectedCount(), the number removeStatisticalOutliers(k, radius, std_mul)
// removed and the points left to <out>.counts (5 x u64), the first call's moments to <out>.moments (3 x double) and the
// coordinates left, extracted, to <out>.xyz.  Exit 8: the selection was not gone after removeStatisticalOutliers.
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

static bool same_file(const std::string& path, const void* p, size_t bytes) {
    std::vector<char> ref(bytes);
    FILE* g = fopen(path.c_str(), "rb");
    if (!g || fread(ref.data(), 1, bytes, g) != bytes) exit(2);
    fclose(g);
    return memcmp(p, ref.data(), bytes) == 0;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    unsigned long long n = 0;
    if (!f || fread(&n, 8, 1, f) != 1) return 2;
    std::vector<P3> pts(n); std::vector<C3> cols(n);
    if (fread(pts.data(), 12, n, f) != n || fread(cols.data(), 3, n, f) != n) return 2;
    fclose(f);
    float r; uint32_t k; double mul;
    f = fopen(argv[2], "rb");
    if (!f || fread(&r, 4, 1, f) != 1 || fread(&k, 4, 1, f) != 1 || fread(&mul, 8, 1, f) != 1) return 2;
    fclose(f);
    const std::string want = argv[3], out = argv[4];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        std::vector<uint32_t> words((size_t)((n + 31) / 32)), found(n);
        std::vector<float> mean(n);
        double moments[3] = {-1, -1, -1};
        auto same_as = [&](const char* ext) {
            if (rtr_download_buffer(pc.context(), RTR_BUF_SELECTION, words.data(), words.size() * 4) != RTR_OK) exit(4);
            return same_file(want + ext, words.data(), words.size() * 4);
        };
        uint64_t counts[5];
        counts[0] = pc.selectStatistical(k, r, mul, RTR_SELECT_REPLACE, false, mean.data(), found.data(), moments);
        if (!same_as(".words0")) return 10;
        if (!same_file(want + ".mean", mean.data(), n * 4)) return 20;
        if (!same_file(want + ".found", found.data(), n * 4)) return 21;
        counts[1] = pc.selectStatistical(k, r, mul, RTR_SELECT_TOGGLE, true);
        if (!same_as(".words1")) return 11;
        counts[2] = pc.selectedCount();
        counts[3] = pc.removeStatisticalOutliers(k, r, mul);
        int set = 1;
        if (rtr_get_option(pc.context(), "selection", &set) != RTR_OK || set != 0 || pc.selectedCount() != 0) return 8;
        rtr_num_points(pc.context(), &counts[4]);
        dump(out + ".counts", counts, sizeof counts);
        dump(out + ".moments", moments, sizeof moments);
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
