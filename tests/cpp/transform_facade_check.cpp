// transformPoints of include/rtr_project_cloud.hpp (rtr.h section 2d) over the C ABI, built with plain g++.  The
// stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   transform_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <M1 16 doubles .bin> <out_prefix>
// The constructor takes a grid of every point (two blocks, the second one scan); transformPoints moves the second block
// [n / 2, n) by M1 (one re-registered scan), then vertices [1000, 1000 + 5000) by M1 again.  Writes <out>.rgb/.depth
// (computeRGBD), <out>.frgb/.fdepth (computeFilteredRGBD).  Exit 7/8: a bad bottom row / range was not refused.
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
    if (argc < 7) { fprintf(stderr, "usage\n"); return 2; }
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
    double M1[16];
    f = fopen(argv[5], "rb");
    if (!f || fread(M1, 8, 16, f) != 16) return 2;
    fclose(f);
    cal.w = W; cal.h = H;
    std::string out = argv[6];
    try {
        std::map<int, Block> grid;  // two blocks: [0, n / 2) and [n / 2, n), flattened in key order
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid);
        pc.transformPoints(M1, n / 2);
        pc.transformPoints(M1, 1000, 5000);
        Img rgb, depth;
        rgb.bytes.resize((size_t)W * H * 3); depth.bytes.resize((size_t)W * H * 4);
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".rgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".depth", depth.bytes.data(), depth.bytes.size());
        if (pc.computeFilteredRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".frgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".fdepth", depth.bytes.data(), depth.bytes.size());
        bool threw = false;  // (a projective bottom row is refused)
        double P4[16];
        for (int i = 0; i < 16; ++i) P4[i] = M1[i];
        P4[14] = 0.5;
        try { pc.transformPoints(P4); } catch (const std::invalid_argument&) { threw = true; }
        if (!threw) return 7;
        for (uint64_t bad : {(uint64_t)n + 1, (uint64_t)n / 2}) {  // (a range past the vertex count is refused)
            threw = false;
            try { pc.transformPoints(M1, bad, n); } catch (const std::out_of_range&) { threw = true; }
            if (!threw) return 8;
        }
        pc.transformPoints(M1, n, 0);  // (an empty range at the end: nothing)
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
