// Host-side C++ check of the facade's several-views methods (include/rtr_project_cloud.hpp, rtr.h section 6c):
// builds with plain g++, links librtr_hip.so.  Stand-in input types as in facade_check.cpp.
//   views_check <cloud.bin> <W> <H> <K9 + 2 x E16 doubles .bin> <out_prefix>
// cloud.bin: u64 n, n*(3 f32), n*(3 u8).  Writes <out>.rgb / .depth (two views, unfiltered) and .frgb / .fdepth.
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

static void dump(const std::string& path, const std::vector<Img>& imgs) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    for (const auto& im : imgs)
        if (fwrite(im.bytes.data(), 1, im.bytes.size(), f) != im.bytes.size()) { perror(path.c_str()); exit(2); }
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    unsigned long long n = 0;
    if (!f || fread(&n, 8, 1, f) != 1) return 2;
    std::map<int, Block> grid;
    std::vector<P3> pts(n); std::vector<C3> cols(n);
    if (fread(pts.data(), 12, n, f) != n || fread(cols.data(), 3, n, f) != n) return 2;
    fclose(f);
    for (unsigned long long i = 0; i < n; ++i) {
        Block& b = grid[i < n / 2 ? 0 : 1];
        b.positions.push_back(pts[i]); b.colors.push_back(cols[i]);
    }
    const int W = atoi(argv[2]), H = atoi(argv[3]);
    Calib cal; std::vector<M44> E(2);
    f = fopen(argv[4], "rb");
    if (!f || fread(cal.K.m, 8, 9, f) != 9 || fread(E[0].m, 8, 16, f) != 16 || fread(E[1].m, 8, 16, f) != 16) return 2;
    fclose(f);
    cal.w = W; cal.h = H;
    const std::string out = argv[5];
    try {
        rtr::ProjectCloud pc(grid, "");
        std::vector<Img> rgb(2), depth(2);
        for (int v = 0; v < 2; ++v) rgb[v].bytes.resize((size_t)W * H * 3), depth[v].bytes.resize((size_t)W * H * 4);
        std::vector<Img*> none(2, nullptr), c{&rgb[0], &rgb[1]}, d{&depth[0], &depth[1]};
        if (pc.computeRGBDViews(cal, E, none, none) != -1) return 3;
        if (pc.computeRGBDViews(cal, E, c, d) != 1) return 3;
        dump(out + ".rgb", rgb);
        dump(out + ".depth", depth);
        if (pc.computeFilteredRGBDViews(cal, E, c, d) != 1) return 3;
        dump(out + ".frgb", rgb);
        dump(out + ".fdepth", depth);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
