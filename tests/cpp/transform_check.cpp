// The arithmetic of rtr_transform_points (csrc/rtr_chunk_box.h, affine_apply) on the host, built with g++
// -ffp-contract=off: reads records of 15 float32 -- the row-major 3 x 4 matrix, then x, y, z -- and writes x', y', z' of
// each as float32 for tests/test_transform_host.py to compare with numpy's float32 arithmetic.
//   transform_check <in.bin> <out.bin>      prints "ok <records>"
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtr_chunk_box.h"

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: transform_check <in.bin> <out.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> in;
    float buf[15 * 4096];
    size_t got;
    while ((got = fread(buf, sizeof(float), 15 * 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    if (in.size() % 15) { fprintf(stderr, "truncated input\n"); return 2; }
    const size_t n = in.size() / 15;
    std::vector<float> out(3 * n);
    for (size_t i = 0; i < n; ++i) {
        rtr::Affine a;
        memcpy(a.m, &in[15 * i], sizeof a.m);
        float x = in[15 * i + 12], y = in[15 * i + 13], z = in[15 * i + 14];
        rtr::affine_apply(a, x, y, z);
        out[3 * i] = x, out[3 * i + 1] = y, out[3 * i + 2] = z;
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) { perror(argv[2]); return 2; }
    fclose(f);
    printf("ok %zu\n", n);
    return 0;
}
