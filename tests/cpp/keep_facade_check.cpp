// The keep-mask methods of include/rtr_project_cloud.hpp (setPointKeep / hidePoints / clearPointKeep, rtr.h section 6e)
// over the C ABI, built with plain g++.  The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   keep_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <keep: n u8 .bin> <hide: u64 count + indices .bin> <out_prefix>
// Writes <out>.set.rgb/.set.depth (setPointKeep), <out>.hide.frgb/.hide.fdepth (hidePoints on top of it, filtered),
// <out>.mask (RTR_BUF_POINT_KEEP after hidePoints) and <out>.clear.rgb/.clear.depth (after clearPointKeep).
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
    if (argc < 8) { fprintf(stderr, "usage\n"); return 2; }
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
    int W = atoi(argv[2]), H = atoi(argv[3]);
    Calib cal; M44 E;
    f = fopen(argv[4], "rb");
    if (!f || fread(cal.K.m, 8, 9, f) != 9 || fread(E.m, 8, 16, f) != 16) return 2;
    fclose(f);
    std::vector<uint8_t> keep(n);
    f = fopen(argv[5], "rb");
    if (!f || fread(keep.data(), 1, n, f) != n) return 2;
    fclose(f);
    unsigned long long nh = 0;
    f = fopen(argv[6], "rb");
    if (!f || fread(&nh, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> hide(nh);
    if (fread(hide.data(), 8, nh, f) != nh) return 2;
    fclose(f);
    cal.w = W; cal.h = H;
    std::string out = argv[7];
    try {
        rtr::ProjectCloud pc(grid, "", 0, true);  // (point_ids: the grid's vertex order, whatever the sort)
        Img rgb, depth;
        rgb.bytes.resize((size_t)W * H * 3); depth.bytes.resize((size_t)W * H * 4);
        pc.setPointKeep(keep);
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".set.rgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".set.depth", depth.bytes.data(), depth.bytes.size());
        pc.hidePoints(hide);
        if (pc.computeFilteredRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".hide.frgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".hide.fdepth", depth.bytes.data(), depth.bytes.size());
        std::vector<uint32_t> words((size_t)((n + 31) / 32));
        if (rtr_download_buffer(pc.context(), RTR_BUF_POINT_KEEP, words.data(), words.size() * 4) != RTR_OK) return 4;
        dump(out + ".mask", words.data(), words.size() * 4);
        bool threw = false;
        try { pc.setPointKeep(std::vector<uint8_t>(n + 1, 1)); } catch (const std::exception&) { threw = true; }
        if (!threw) return 7;
        threw = false;
        try { pc.hidePoints({n}); } catch (const std::exception&) { threw = true; }
        if (!threw) return 7;
        pc.clearPointKeep();
        int set = 1;
        if (rtr_get_option(pc.context(), "point_keep", &set) != RTR_OK || set != 0) return 4;
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".clear.rgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".clear.depth", depth.bytes.data(), depth.bytes.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
