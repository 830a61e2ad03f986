// fitPlane / selectPlane / segmentPlane / countInBands of include/rtr_project_cloud.hpp (rtr.h section 6j) over the C
// ABI, built with plain g++.  The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   planes_facade_check <cloud.bin> <args: dist f32, iterations u32, seed u64 .bin> <out_prefix>
// fitPlane -> <out>.fit0 (4 x f32 plane, then 5 x u64: inliers and the four stats); selectPlane of it -> <out>.words0 and
// its count; segmentPlane -> <out>.words1; the selection toggled (everything but the plane) and fitPlane(selected) ->
// <out>.fit1; countInBands of that plane's band over the selected vertices -> its count.  <out>.counts (4 x u64):
// selectPlane's count, segmentPlane's inliers, the toggled count, the band count.  Exit 8: fitPlane changed the selection
// or did not throw on a cloud of two vertices.
#include <cstdio>
#include <cstdlib>
#include <map>
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
static void dump_fit(const std::string& path, const rtr::ProjectCloud::Plane& p, const uint64_t st[4]) {
    unsigned char rec[16 + 40];
    const uint64_t five[5] = {p.inliers, st[0], st[1], st[2], st[3]};
    memcpy(rec, p.abcd, 16);
    memcpy(rec + 16, five, 40);
    dump(path, rec, sizeof rec);
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    unsigned long long n = 0;
    if (!f || fread(&n, 8, 1, f) != 1) return 2;
    std::vector<P3> pts(n); std::vector<C3> cols(n);
    if (fread(pts.data(), 12, n, f) != n || fread(cols.data(), 3, n, f) != n) return 2;
    fclose(f);
    float dist = 0.f;
    uint32_t iterations = 0;
    uint64_t seed = 0;
    f = fopen(argv[2], "rb");
    if (!f || fread(&dist, 4, 1, f) != 1 || fread(&iterations, 4, 1, f) != 1 || fread(&seed, 8, 1, f) != 1) return 2;
    fclose(f);
    std::string out = argv[3];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        std::vector<uint32_t> words((size_t)((n + 31) / 32));
        auto words_to = [&](const char* ext) {
            if (rtr_download_buffer(pc.context(), RTR_BUF_SELECTION, words.data(), words.size() * 4) != RTR_OK) exit(4);
            dump(out + ext, words.data(), words.size() * 4);
        };
        uint64_t counts[4], st[4];
        int set = 1;
        const rtr::ProjectCloud::Plane p0 = pc.fitPlane(dist, iterations, seed, false, st);
        dump_fit(out + ".fit0", p0, st);
        if (rtr_get_option(pc.context(), "selection", &set) != RTR_OK || set != 0) return 8;  // (no selection was created)
        counts[0] = pc.selectPlane(p0.abcd, dist);
        words_to(".words0");
        pc.clearSelection();
        counts[1] = pc.segmentPlane(dist, iterations, seed).inliers;
        words_to(".words1");
        uint64_t toggled[4];
        if (rtr_select_points(pc.context(), 0, nullptr, nullptr, nullptr, RTR_SELECT_TOGGLE, toggled) != RTR_OK) return 4;
        counts[2] = toggled[0];
        const rtr::ProjectCloud::Plane p1 = pc.fitPlane(dist, iterations, seed + 1, true, st);
        dump_fit(out + ".fit1", p1, st);
        if (pc.selectedCount() != counts[2]) return 8;
        const float band[5] = {p1.abcd[0], p1.abcd[1], p1.abcd[2], p1.abcd[3] + dist, dist - p1.abcd[3]};
        counts[3] = pc.countInBands(band, 1, true)[0];
        dump(out + ".counts", counts, sizeof counts);
        // every candidate degenerate: the facade throws
        std::map<int, Block> two;
        two[0].positions.assign(pts.begin(), pts.begin() + 2);
        two[0].colors.assign(cols.begin(), cols.begin() + 2);
        rtr::ProjectCloud tiny(two, "", 0, true);
        bool threw = false;
        try { tiny.fitPlane(dist, iterations, seed); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) return 8;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
