// selectNear / appendNewPoints of include/rtr_project_cloud.hpp (rtr.h section 6k) over the C ABI, built with plain g++.
// The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   near_facade_check <cloud.bin> <given.bin> <params: radius, radius2 as 2 floats .bin> <want_prefix> <out_prefix>
// cloud.bin / given.bin: a u64 count, that many tight xyz, that many tight rgb.  <want>.words0 / .words1 hold the words
// the reference expects after: selectNear(given, radius) with near words; selectNear(given, radius2, ADD, outside).  The
// program compares the selection after each step with them (exit 10 + step on a difference) and the near words of step 0
// with <want>.near (exit 13), then appendNewPoints(given, radius): exit 8 when the selection changed with it.  It writes
// the two counts, selectedCount(), the number appended and the points then resident to <out>.counts (5 x u64) and the
// appended coordinates, extracted, to <out>.xyz.
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
static void load(const char* path, std::vector<P3>& pts, std::vector<C3>& cols) {
    FILE* f = fopen(path, "rb");
    unsigned long long n = 0;
    if (!f || fread(&n, 8, 1, f) != 1) exit(2);
    pts.resize(n); cols.resize(n);
    if (fread(pts.data(), 12, n, f) != n || fread(cols.data(), 3, n, f) != n) exit(2);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage\n"); return 2; }
    std::vector<P3> pts, given; std::vector<C3> cols, gcols;
    load(argv[1], pts, cols);
    load(argv[2], given, gcols);
    const size_t n = pts.size(), m = given.size();
    float r[2];
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(r, 4, 2, f) != 2) return 2;
    fclose(f);
    const std::string want = argv[4], out = argv[5];
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
        std::vector<uint32_t> near, near_ref((m + 31) / 32);
        counts[0] = pc.selectNear(&given[0].x, 12, m, r[0], RTR_SELECT_REPLACE, false, &near);
        if (!same_as(".words0")) return 10;
        FILE* g = fopen((want + ".near").c_str(), "rb");
        if (!g || fread(near_ref.data(), 4, near_ref.size(), g) != near_ref.size()) return 2;
        fclose(g);
        if (near != near_ref) return 13;
        counts[1] = pc.selectNear(&given[0].x, 12, m, r[1], RTR_SELECT_ADD, true);
        if (!same_as(".words1")) return 11;
        counts[2] = pc.selectedCount();
        // a scan that adds points drops the selection with the append (section 6f); one that adds nothing leaves it alone
        counts[3] = pc.appendNewPoints(&given[0].x, 12, &gcols[0].v[0], 3, m, r[0]);
        rtr_num_points(pc.context(), &counts[4]);
        if (pc.appendNewPoints(&given[0].x, 12, &gcols[0].v[0], 3, m, r[0]) != 0) return 8;  // (every given point is resident now)
        dump(out + ".counts", counts, sizeof counts);
        std::vector<float> xyz; std::vector<uint8_t> rgb;
        pc.extractAll(xyz, rgb);
        dump(out + ".xyz", xyz.data() + 3 * n, (xyz.size() - 3 * n) * 4);
        dump(out + ".rgb", rgb.data() + 3 * n, rgb.size() - 3 * n);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
