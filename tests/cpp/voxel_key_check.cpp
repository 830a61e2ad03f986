// rtr::voxel_key of csrc/rtr_voxel_key.h (rtr.h section 6g) built with plain g++ -ffp-contract=off -fno-fast-math: the
// cell arithmetic the key kernel runs, on the host.  A stand-alone program, so it also builds with
// -fsanitize=address,undefined.
//   voxel_key_check <in.bin> <out.bin>
// in: origin (3 floats), cell (3 floats), n (u64), n x 3 floats.  out: n x u64 keys, inv = 1.0f / cell as the library
// computes it.  Prints "ok <n> <points out of the grid>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rtr_voxel_key.h"

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: voxel_key_check in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    float origin[3], cell[3], inv[3];
    unsigned long long n = 0;
    if (!f || fread(origin, 4, 3, f) != 3 || fread(cell, 4, 3, f) != 3 || fread(&n, 8, 1, f) != 1) return 2;
    std::vector<float> xyz((size_t)n * 3);
    if (fread(xyz.data(), 12, n, f) != n) return 2;
    fclose(f);
    for (int k = 0; k < 3; ++k) inv[k] = 1.0f / cell[k];
    std::vector<uint64_t> keys((size_t)n);
    unsigned long long out = 0;
    for (size_t i = 0; i < n; ++i) {
        keys[i] = rtr::voxel_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], origin, inv);
        out += (keys[i] & rtr::kVoxelOut) != 0;
        if ((keys[i] & rtr::kVoxelOut) && keys[i] != rtr::kVoxelOut) return 3;  // (the low bits are the kernel's to fill)
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(keys.data(), 8, n, f) != n) return 2;
    fclose(f);
    printf("ok %llu %llu\n", n, out);
    return 0;
}
