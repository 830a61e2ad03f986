// rtr::ProjectCloud::computePointIds / visible_points (include/rtr_project_cloud.hpp) with plain g++ against
// librtr_hip.so; the stand-in types are test input types with the members the facade uses (see facade_check.cpp).
//   point_ids_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <out_prefix>
// cloud.bin: u64 n, n*(3 f32), n*(3 u8).  Writes <out>.ids (i64 [H*W]) and <out>.vis (u8 [n]), unfiltered frame.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "rtr_project_cloud.hpp"

struct P3 { float x, y, z; };
struct C3 { unsigned char v[3]; unsigned char operator[](int i) const { return v[i]; } };
struct Block { std::vector<P3> positions; std::vector<C3> colors; };
struct K33 { double m[9]; double operator()(int r, int c) const { return m[3 * r + c]; } };
struct M44 { double m[16]; double operator()(int r, int c) const { return m[4 * r + c]; } };
struct Calib {
    K33 K; int w, h;
    int getWidth() const { return w; }
    int getHeight() const { return h; }
    K33 getIntrinsicsMatrix() const { return K; }
};

static void dump(const std::string& path, const void* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { perror(path.c_str()); exit(2); }
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    unsigned long long n = 0;
    if (!f || fread(&n, 8, 1, f) != 1) return 2;
    std::vector<P3> pts(n); std::vector<C3> cols(n);
    if (fread(pts.data(), 12, n, f) != n || fread(cols.data(), 3, n, f) != n) return 2;
    fclose(f);
    std::map<int, Block> grid;  // two blocks in order: the flattened vertex order is the file's
    for (unsigned long long i = 0; i < n; ++i) {
        Block& b = grid[i < n / 2 ? 0 : 1];
        b.positions.push_back(pts[i]); b.colors.push_back(cols[i]);
    }
    Calib cal; M44 E;
    f = fopen(argv[4], "rb");
    if (!f || fread(cal.K.m, 8, 9, f) != 9 || fread(E.m, 8, 16, f) != 16) return 2;
    fclose(f);
    cal.w = atoi(argv[2]); cal.h = atoi(argv[3]);
    const std::string out = argv[5];
    try {
        rtr::ProjectCloud pc(grid, "", 0, true);
        const std::vector<int64_t> ids = pc.computePointIds(cal, E);
        const std::vector<uint8_t> vis = pc.visible_points(cal, E);
        if (ids.size() != (size_t)cal.w * cal.h || vis.size() != n) return 3;
        dump(out + ".ids", ids.data(), ids.size() * 8);
        dump(out + ".vis", vis.data(), vis.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
