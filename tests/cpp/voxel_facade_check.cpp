// selectVoxelGrid / thin of include/rtr_project_cloud.hpp (rtr.h section 6g) over the C ABI, built with plain g++.  The
// stand-in types are the TEST INPUT TYPES of facade_check.cpp.
//   voxel_facade_check <cloud.bin> <W> <H> <K9+E16 doubles .bin> <grid: cell 3 floats, origin 3 floats, thin cell .bin> <out_prefix>
// Selects one vertex per cell (<out>.words0), the cells with at least 3 vertices (<out>.words1), adds everything but the
// representatives of the first call (<out>.words2: every vertex that is no representative, or one of a full cell) and
// writes the counts after each step and selectedCount() to <out>.counts (4 x u64); then thins the cloud by the thin
// cell: <out>.n (the vertices left, twice: thin's return value and rtr_num_points) and the frame <out>.rgb / .depth.
// Exit 8: the selection was not gone after thin.
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
    float g[7];
    f = fopen(argv[5], "rb");
    if (!f || fread(g, 4, 7, f) != 7) return 2;
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
        std::vector<uint32_t> words((size_t)((n + 31) / 32));
        auto words_to = [&](const char* ext) {
            if (rtr_download_buffer(pc.context(), RTR_BUF_SELECTION, words.data(), words.size() * 4) != RTR_OK) exit(4);
            dump(out + ext, words.data(), words.size() * 4);
        };
        uint64_t counts[4];
        counts[0] = pc.selectVoxelGrid(g, g + 3);
        words_to(".words0");
        counts[1] = pc.selectVoxelGrid(g, g + 3, 3);
        words_to(".words1");
        counts[2] = pc.selectVoxelGrid(g, g + 3, 1, RTR_SELECT_ADD, true);
        words_to(".words2");
        counts[3] = pc.selectedCount();
        dump(out + ".counts", counts, sizeof counts);
        uint64_t left[2] = {pc.thin(g[6]), 0};
        int set = 1;
        if (rtr_get_option(pc.context(), "selection", &set) != RTR_OK || set != 0 || pc.selectedCount() != 0) return 8;
        rtr_num_points(pc.context(), &left[1]);
        dump(out + ".n", left, sizeof left);
        Img rgb, depth;
        rgb.bytes.resize((size_t)W * H * 3); depth.bytes.resize((size_t)W * H * 4);
        if (pc.computeRGBD(cal, E, &rgb, &depth) != 1) return 3;
        dump(out + ".rgb", rgb.bytes.data(), rgb.bytes.size());
        dump(out + ".depth", depth.bytes.data(), depth.bytes.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    return 0;
}
