// nearestKPoints of include/rtr_project_cloud.hpp (rtr.h section 6m) over the C ABI, built with plain g++.
// The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   nearest_k_facade_check <cloud.bin> <given.bin> <params: radius as 1 float, k as 1 u32 .bin> <want_prefix> <out_prefix>
// cloud.bin / given.bin: a u64 count, that many tight xyz, that many tight rgb.  <want>.index / .dist2 hold the m * k upload
// indices and squared distances (as bits), <want>.found the m counts the reference expects of nearestKPoints(given, k,
// radius); the program compares (exit 10 / 11 / 12 on a difference) and writes the sum of found to <out>.counts (1 x u64).
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
static void want_words(const std::string& path, std::vector<uint32_t>& w) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f || fread(w.data(), 4, w.size(), f) != w.size()) exit(2);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage\n"); return 2; }
    std::vector<P3> pts, given; std::vector<C3> cols, gcols;
    load(argv[1], pts, cols);
    load(argv[2], given, gcols);
    const size_t n = pts.size(), m = given.size();
    float r = 0.f;
    uint32_t k = 0;
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(&r, 4, 1, f) != 1 || fread(&k, 4, 1, f) != 1) return 2;
    fclose(f);
    const std::string want = argv[4], out = argv[5];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        std::vector<uint32_t> idx(m * k), d2(m * k), found(m);
        want_words(want + ".index", idx);
        want_words(want + ".dist2", d2);
        want_words(want + ".found", found);
        const rtr::ProjectCloud::NearestK nn = pc.nearestKPoints(&given[0].x, 12, m, k, r);
        if (nn.k != k || nn.index != idx) return 10;
        if (nn.dist2.size() != m * k || memcmp(nn.dist2.data(), d2.data(), 4 * m * k) != 0) return 11;
        if (nn.found != found) return 12;
        uint64_t total = 0;
        for (size_t j = 0; j < m; ++j) total += nn.found[j];
        dump(out + ".counts", &total, sizeof total);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
