// registerPoints of include/rtr_project_cloud.hpp (rtr_register.h section 6p) over the C ABI, built with plain g++.  The
// stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   register_facade_check <cloud.bin> <scan: u64 m, then m x 3 floats .bin> <params: radius as 1 float .bin> <out_prefix>
// The program calls registerPoints(scan, 12, m, radius) and registerPoints(scan, 12, m, radius, 20, true) -- the facade
// estimates the normals itself -- and writes per mode <out>.pose<mode> (16 doubles), <out>.rms<mode> and <out>.stats<mode>
// (4 x u64).  Exit 8: a call created a selection.
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
    unsigned long long n = 0, m = 0;
    if (!f || fread(&n, 8, 1, f) != 1) return 2;
    std::vector<P3> pts(n); std::vector<C3> cols(n);
    if (fread(pts.data(), 12, n, f) != n || fread(cols.data(), 3, n, f) != n) return 2;
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f || fread(&m, 8, 1, f) != 1) return 2;
    std::vector<float> scan(3 * m);
    if (fread(scan.data(), 12, m, f) != m) return 2;
    fclose(f);
    float r;
    f = fopen(argv[3], "rb");
    if (!f || fread(&r, 4, 1, f) != 1) return 2;
    fclose(f);
    const std::string out = argv[4];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        static_assert(RTR_REGISTER_POINT_TO_PLANE == 1 && RTR_REGISTER_MOMENTS == 32, "rtr_register.h through the facade");
        const std::vector<float> before = scan;
        for (int mode = 0; mode < 2; ++mode) {
            const rtr::ProjectCloud::Registration reg = pc.registerPoints(scan.data(), 12, m, r, 20, mode != 0);
            const std::string tag = std::to_string(mode);
            dump(out + ".pose" + tag, reg.pose, sizeof reg.pose);
            dump(out + ".rms" + tag, reg.rms.data(), reg.rms.size() * sizeof(double));
            dump(out + ".stats" + tag, reg.stats, sizeof reg.stats);
        }
        int set = 1;
        if (rtr_get_option(pc.context(), "selection", &set) != RTR_OK || set != 0) return 8;
        if (scan != before) return 9;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
