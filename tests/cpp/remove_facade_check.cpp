// removePoints / commitPointKeep of include/rtr_project_cloud.hpp (rtr.h section 2c) over the C ABI, built with plain
// g++.  The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   remove_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <out_prefix>
// The constructor takes a grid of every point (two blocks); removePoints takes out the vertices whose index is a
// multiple of 3; setPointKeep hides every 5th of the survivors (new indices) and commitPointKeep removes them.  Writes
// <out>.rgb/.depth (computeRGBD), <out>.frgb/.fdepth (computeFilteredRGBD) and <out>.n (the resident point count, u64).
#include <cstdio>
#include <cstdlib>
#include <map>
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
struct Img {
    std::vector<unsigned char> bytes;
    template <class T> T* ptr() { return reinterpret_cast<T*>(bytes.data()); }
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
    int W = atoi(argv[2]), H = atoi(argv[3]);
    Calib cal; M44 E;
    f = fopen(argv[4], "rb");
    if (!f || fread(cal.K.m, 8, 9, f) != 9 || fread(E.m, 8, 16, f) != 16) return 2;
    fclose(f);
    cal.w = W; cal.h = H;
    std::string out = argv[5];
    try {
        std::map<int, Block> grid;  // two blocks: [0, n / 2) and [n / 2, n), flattened in key order
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid);
        std::vector<uint64_t> gone;
        for (uint64_t i = 0; i < n; i += 3) gone.push_back(i);
        pc.removePoints(gone);
        uint64_t m = 0;
        if (rtr_num_points(pc.context(), &m) != RTR_OK || m != n - gone.size()) return 4;
        pc.commitPointKeep();  // (no mask: nothing)
        std::vector<uint8_t> keep((size_t)m, 1);
        for (size_t i = 0; i < keep.size(); i += 5) keep[i] = 0;
        pc.setPointKeep(keep);
        pc.commitPointKeep();
        int set = 1;
        if (rtr_get_option(pc.context(), "point_keep", &set) != RTR_OK || set != 0) return 6;
        uint64_t count = 0;
        if (rtr_num_points(pc.context(), &count) != RTR_OK) return 4;
        dump(out + ".n", &count, 8);
        Img rgb, depth;
        rgb.bytes.resize((size_t)W * H * 3); depth.bytes.resize((size_t)W * H * 4);
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".rgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".depth", depth.bytes.data(), depth.bytes.size());
        if (pc.computeFilteredRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".frgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".fdepth", depth.bytes.data(), depth.bytes.size());
        bool threw = false;  // (an index past the count is refused)
        try { pc.removePoints({count}); } catch (const std::exception&) { threw = true; }
        if (!threw) return 7;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
