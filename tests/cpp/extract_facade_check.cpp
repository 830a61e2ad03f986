// extractSelected / extractAll of include/rtr_project_cloud.hpp (rtr.h section 2e) over the C ABI, built with plain g++.
// The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   extract_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <box 6 floats .bin> <out_prefix>
// Selects the box, extracts the selection with indices (<out>.xyz: 3 floats per vertex, <out>.rgb: 3 bytes, <out>.idx,
// <out>.counts: selectBox's count, extractSelected's, extractAll's), builds a SECOND cloud from the extracted vectors
// (an empty grid, then appendPoints with the tight strides) and renders one frame of it (<out>.rgbimg / .depth).
// Exit 6: extractAll did not give the cloud back, 7: a cloud without a selection did not extract nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    float box[6];
    f = fopen(argv[5], "rb");
    if (!f || fread(box, 4, 6, f) != 6) return 2;
    fclose(f);
    cal.w = W; cal.h = H;
    std::string out = argv[6];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        std::vector<float> xyz;
        std::vector<uint8_t> rgb;
        std::vector<uint32_t> idx;
        if (pc.extractSelected(xyz, rgb, &idx) != 0 || !xyz.empty() || !rgb.empty() || !idx.empty()) return 7;
        uint64_t counts[3];
        counts[0] = pc.selectBox(box, box + 3);
        counts[1] = pc.extractSelected(xyz, rgb, &idx);
        if (xyz.size() != counts[1] * 3 || rgb.size() != counts[1] * 3 || idx.size() != counts[1]) return 3;
        dump(out + ".xyz", xyz.data(), xyz.size() * 4);
        dump(out + ".rgb", rgb.data(), rgb.size());
        dump(out + ".idx", idx.data(), idx.size() * 4);
        std::vector<float> all_xyz;
        std::vector<uint8_t> all_rgb;
        counts[2] = pc.extractAll(all_xyz, all_rgb);
        dump(out + ".counts", counts, sizeof counts);
        if (counts[2] != n || memcmp(all_xyz.data(), pts.data(), n * 12) != 0 || memcmp(all_rgb.data(), cols.data(), n * 3) != 0) return 6;
        if (pc.selectedCount() != counts[0]) return 3;  // (the selection is still there)
        std::map<int, Block> none;
        rtr::ProjectCloud second(none);
        second.appendPoints(xyz.data(), 12, rgb.data(), 3, (size_t)counts[1]);
        Img img, depth;
        img.bytes.resize((size_t)W * H * 3); depth.bytes.resize((size_t)W * H * 4);
        if (second.computeRGBD(cal, E, &img, &depth) != 1) return 3;
        dump(out + ".rgbimg", img.bytes.data(), img.bytes.size());
        dump(out + ".depth", depth.bytes.data(), depth.bytes.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
