// writeSelected / writePoints / colorSelected of include/rtr_project_cloud.hpp (rtr.h section 2f) over the C ABI, built
// with plain g++.  The stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   write_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <box 6 floats .bin> <out_prefix>
// Selects the box, extracts the selection, edits it (vertex j: x + 0.25, y, z - 0.5; colour j: 255 - c) and writes it
// back with writeSelected; then writePoints gives the vertices [7, 7 + 300) the first 300 edited records (vertices only),
// and colorSelected paints the selection (10, 200, 30).  After each step one frame (<out>.rgbimg<k> / .depth<k>, k = 0,
// 1, 2) and at the end extractAll (<out>.xyz / .rgb) and <out>.counts: selectBox's count and the three calls' returns.
// Exit 6: the selection did not survive, 7: an argument rule did not throw.
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

template <class Fn>
static bool throws_invalid(Fn fn) {
    try { fn(); } catch (const std::invalid_argument&) { return true; } catch (const std::out_of_range&) { return true; }
    return false;
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
        Img img, depth;
        img.bytes.resize((size_t)W * H * 3); depth.bytes.resize((size_t)W * H * 4);
        auto frame = [&](const char* k) {
            if (pc.computeRGBD(cal, E, &img, &depth) != 1) exit(3);
            dump(out + ".rgbimg" + k, img.bytes.data(), img.bytes.size());
            dump(out + ".depth" + k, depth.bytes.data(), depth.bytes.size());
        };
        std::vector<float> xyz, none_xyz;
        std::vector<uint8_t> rgb, none_rgb;
        uint64_t counts[4];
        if (pc.writeSelected(std::vector<float>(3, 0.f), none_rgb) != 0 || pc.colorSelected(1, 2, 3) != 0) return 6;  // (no selection yet)
        counts[0] = pc.selectBox(box, box + 3);
        if (pc.extractSelected(xyz, rgb) != counts[0] || counts[0] < 400) return 3;
        for (size_t j = 0; j < counts[0]; ++j) {
            xyz[3 * j] += 0.25f, xyz[3 * j + 2] -= 0.5f;
            for (int c = 0; c < 3; ++c) rgb[3 * j + c] = (uint8_t)(255 - rgb[3 * j + c]);
        }
        if (!throws_invalid([&] { pc.writeSelected(std::vector<float>(4, 0.f), none_rgb); })) return 7;
        if (!throws_invalid([&] { pc.writeSelected(none_xyz, std::vector<uint8_t>(5, 0)); })) return 7;
        if (!throws_invalid([&] { pc.writeSelected(std::vector<float>(6, 0.f), std::vector<uint8_t>(3, 0)); })) return 7;
        if (!throws_invalid([&] { pc.writeSelected(none_xyz, none_rgb); })) return 7;
        if (!throws_invalid([&] { pc.writePoints(n - 1, 2, std::vector<float>(6, 0.f), none_rgb); })) return 7;
        if (!throws_invalid([&] { pc.writePoints(0, 3, std::vector<float>(6, 0.f), none_rgb); })) return 7;
        counts[1] = pc.writeSelected(xyz, rgb);
        frame("0");
        std::vector<float> head(xyz.begin(), xyz.begin() + 900);
        counts[2] = pc.writePoints(7, 300, head, none_rgb);
        frame("1");
        counts[3] = pc.colorSelected(10, 200, 30);
        frame("2");
        if (pc.selectedCount() != counts[0]) return 6;  // (the selection is still there, naming the same vertices)
        dump(out + ".counts", counts, sizeof counts);
        std::vector<float> all_xyz;
        std::vector<uint8_t> all_rgb;
        if (pc.extractAll(all_xyz, all_rgb) != n) return 3;
        dump(out + ".xyz", all_xyz.data(), all_xyz.size() * 4);
        dump(out + ".rgb", all_rgb.data(), all_rgb.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
