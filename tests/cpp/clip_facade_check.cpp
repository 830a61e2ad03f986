// The clip methods of include/rtr_project_cloud.hpp (setClipPlanes / setClipBox / clearClip, rtr.h section 6d) over the
// C ABI, built with plain g++.  The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   clip_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <box: 6 f32 .bin> <M: 16 f64 .bin> <out_prefix>
// Writes <out>.box.rgb/.box.depth (axis box), <out>.obox.* (oriented box, M), <out>.plane.frgb/.fdepth/.tensor (one
// plane {0,1,0,0}, filtered), <out>.clear.rgb/.depth (after clearClip) and <out>.planes (the planes read back).
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
    float box[6];
    double M[16];
    f = fopen(argv[5], "rb");
    if (!f || fread(box, 4, 6, f) != 6) return 2;
    fclose(f);
    f = fopen(argv[6], "rb");
    if (!f || fread(M, 8, 16, f) != 16) return 2;
    fclose(f);
    cal.w = W; cal.h = H;
    std::string out = argv[7];
    try {
        rtr::ProjectCloud pc(grid, "");
        Img rgb, depth;
        rgb.bytes.resize((size_t)W * H * 3); depth.bytes.resize((size_t)W * H * 4);
        pc.setClipBox(box, box + 3);
        float pl[8 * 4];
        int count = 0;
        if (rtr_get_clip_planes(pc.context(), &count, pl) != RTR_OK || count != 6) return 4;
        dump(out + ".planes", pl, 6 * 4 * 4);
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".box.rgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".box.depth", depth.bytes.data(), depth.bytes.size());
        pc.setClipBox(box, box + 3, M);
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".obox.rgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".obox.depth", depth.bytes.data(), depth.bytes.size());
        if (rtr_get_clip_planes(pc.context(), &count, pl) != RTR_OK || count != 6) return 4;
        dump(out + ".oplanes", pl, 6 * 4 * 4);
        const float plane[4] = {0.f, 1.f, 0.f, 0.f};
        pc.setClipPlanes(plane, 1);
        if (pc.computeFilteredRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".plane.frgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".plane.fdepth", depth.bytes.data(), depth.bytes.size());
        std::vector<unsigned char> t((size_t)W * H * 10);
        if (rtr_download_buffer(pc.context(), RTR_BUF_TENSOR, t.data(), t.size()) != RTR_OK) return 4;
        dump(out + ".plane.tensor", t.data(), t.size());
        bool threw = false;
        const float bad[4] = {0.f, 0.f, 0.f, 1.f};
        try { pc.setClipPlanes(bad, 1); } catch (const std::exception&) { threw = true; }
        if (!threw) return 7;
        pc.clearClip();
        if (rtr_get_clip_planes(pc.context(), &count, nullptr) != RTR_OK || count != 0) return 4;
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".clear.rgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".clear.depth", depth.bytes.data(), depth.bytes.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
