// appendPoints of include/rtr_project_cloud.hpp (rtr.h section 2b) over the C ABI, built with plain g++.  The stand-in
// types are the TEST INPUT TYPES of facade_check.cpp.
//   append_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <out_prefix>
// The constructor takes a grid of the first third of the points (two blocks), appendPoints(grid) the second third (two
// blocks), the raw-pointer appendPoints the rest (float4 / uchar4).  Writes <out>.rgb/.depth (computeRGBD),
// <out>.frgb/.fdepth (computeFilteredRGBD) and <out>.n (the resident point count, u64).
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

static std::map<int, Block> grid_of(const std::vector<P3>& pts, const std::vector<C3>& cols, size_t a, size_t b) {
    std::map<int, Block> grid;  // two blocks: [a, mid) and [mid, b), flattened in key order
    const size_t mid = a + (b - a) / 2;
    for (size_t i = a; i < b; ++i) {
        Block& blk = grid[i < mid ? 0 : 1];
        blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
    }
    return grid;
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
    const size_t a = n / 3, b = 2 * n / 3;
    try {
        rtr::ProjectCloud pc(grid_of(pts, cols, 0, a));
        pc.appendPoints(grid_of(pts, cols, a, b));
        std::vector<float> xyzw;
        std::vector<uint8_t> rgba;
        for (size_t i = b; i < n; ++i) {
            xyzw.insert(xyzw.end(), {pts[i].x, pts[i].y, pts[i].z, 1.0f});
            rgba.insert(rgba.end(), {cols[i][0], cols[i][1], cols[i][2], 255});
        }
        pc.appendPoints(xyzw.data(), 16, rgba.data(), 4, n - b);
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
        bool threw = false;  // (a bad stride is refused)
        try { pc.appendPoints(xyzw.data(), 8, rgba.data(), 4, 1); } catch (const std::exception&) { threw = true; }
        if (!threw) return 7;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
