// selectBox / selectPlanes / selectRect / removeSelected / hideSelected / transformSelected of
// include/rtr_project_cloud.hpp (rtr.h section 6f) over the C ABI, built with plain g++.  The stand-in types are the
// TEST INPUT TYPES of facade_check.cpp.
//   select_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <M1 16 doubles .bin> <box 6 floats .bin> <out_prefix>
// Selects the box, intersects it with the half-space x >= 0, adds the screen rectangle [W/8, 5W/8) x [H/8, 7H/8) of the
// pose and writes the counts after each step to <out>.counts (4 x u64, the last one selectedCount()) and the selection's
// words to <out>.words; hides the selection (<out>.hrgb / .hdepth), clears the mask, moves the selection by M1
// (<out>.trgb / .tdepth, filtered) and removes it (<out>.rrgb / .rdepth, <out>.n: the vertices left).
// Exit 7: a bad bottom row was not refused, 8: the selection was not gone after removeSelected.
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
    float box[6];
    f = fopen(argv[6], "rb");
    if (!f || fread(box, 4, 6, f) != 6) return 2;
    fclose(f);
    cal.w = W; cal.h = H;
    std::string out = argv[7];
    try {
        std::map<int, Block> grid;
        for (size_t i = 0; i < n; ++i) {
            Block& blk = grid[i < n / 2 ? 0 : 1];
            blk.positions.push_back(pts[i]); blk.colors.push_back(cols[i]);
        }
        rtr::ProjectCloud pc(grid, "", 0, true);
        uint64_t counts[4];
        if (pc.selectedCount() != 0) return 3;
        counts[0] = pc.selectBox(box, box + 3);
        const float half[4] = {1.f, 0.f, 0.f, 0.f};
        counts[1] = pc.selectPlanes(half, 1, RTR_SELECT_INTERSECT);
        counts[2] = pc.selectRect(cal, E, W / 8, H / 8, 5 * W / 8, 7 * H / 8, RTR_SELECT_ADD);
        counts[3] = pc.selectedCount();
        dump(out + ".counts", counts, sizeof counts);
        std::vector<uint32_t> words((size_t)((n + 31) / 32));
        if (rtr_download_buffer(pc.context(), RTR_BUF_SELECTION, words.data(), words.size() * 4) != RTR_OK) return 4;
        dump(out + ".words", words.data(), words.size() * 4);
        Img rgb, depth;
        rgb.bytes.resize((size_t)W * H * 3); depth.bytes.resize((size_t)W * H * 4);
        pc.hideSelected();
        if (pc.selectedCount() != counts[3]) return 3;
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".hrgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".hdepth", depth.bytes.data(), depth.bytes.size());
        pc.clearPointKeep();
        bool threw = false;
        double P4[16];
        for (int i = 0; i < 16; ++i) P4[i] = M1[i];
        P4[14] = 0.5;
        try { pc.transformSelected(P4); } catch (const std::invalid_argument&) { threw = true; }
        if (!threw) return 7;
        pc.transformSelected(M1);
        if (pc.selectedCount() != counts[3]) return 3;
        if (pc.computeFilteredRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".trgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".tdepth", depth.bytes.data(), depth.bytes.size());
        pc.removeSelected();
        int set = 1;
        if (rtr_get_option(pc.context(), "selection", &set) != RTR_OK || set != 0 || pc.selectedCount() != 0) return 8;
        uint64_t left = 0;
        rtr_num_points(pc.context(), &left);
        dump(out + ".n", &left, 8);
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".rrgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".rdepth", depth.bytes.data(), depth.bytes.size());
        pc.clearSelection();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
