// nearestPoints / matchPoints of include/rtr_project_cloud.hpp (rtr.h section 6l) over the C ABI, built with plain g++.
// The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   nearest_facade_check <cloud.bin> <given.bin> <params: radius as 1 float .bin> <want_prefix> <out_prefix>
// cloud.bin / given.bin: a u64 count, that many tight xyz, that many tight rgb.  <want>.index / .dist2 hold the m upload
// indices and the m squared distances (as bits) the reference expects of nearestPoints(given, radius); the program
// compares (exit 10 / 11 on a difference), then matchPoints(given, radius): exit 12 when its index or dist2 differ from
// nearestPoints'.  It writes the matched coordinates and colours to <out>.xyz (3 m floats) and <out>.rgb (3 m bytes) and
// the number of matches to <out>.counts (1 x u64).
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
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(&r, 4, 1, f) != 1) return 2;
    fclose(f);
    const std::string want = argv[4], out = argv[5];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        std::vector<uint32_t> idx(m), d2(m);
        want_words(want + ".index", idx);
        want_words(want + ".dist2", d2);
        const rtr::ProjectCloud::Nearest nn = pc.nearestPoints(&given[0].x, 12, m, r);
        if (nn.index != idx) return 10;
        if (nn.dist2.size() != m || memcmp(nn.dist2.data(), d2.data(), 4 * m) != 0) return 11;
        const rtr::ProjectCloud::Match mt = pc.matchPoints(&given[0].x, 12, m, r);
        if (mt.index != idx || memcmp(mt.dist2.data(), d2.data(), 4 * m) != 0) return 12;
        if (mt.vertices.size() != 3 * m || mt.colors.size() != 3 * m) return 13;
        uint64_t matched = 0;
        for (size_t j = 0; j < m; ++j) matched += mt.index[j] != RTR_NEAREST_NONE;
        dump(out + ".counts", &matched, sizeof matched);
        dump(out + ".xyz", mt.vertices.data(), mt.vertices.size() * 4);
        dump(out + ".rgb", mt.colors.data(), mt.colors.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
