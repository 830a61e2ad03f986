// rtr_chunk_box.h -- the frustum half-spaces and the box of a packed chunk, shared by the point kernel and the host
// (plain C++ apart from the qualifiers: tests/cpp/chunk_box_check.cpp compiles it with g++).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RTR_HD __host__ __device__ inline
#else
#define RTR_HD inline
#endif

namespace rtr {

constexpr uint32_t kPackWideFlag = 1u << 18;  // header widths word: some axis of the chunk needs all 32 bits

// The five half-spaces r.z >= 0, r.x + r.z >= 0, W r.z - r.x >= 0, r.y + r.z >= 0, H r.z - r.y >= 0 (r = the matrix
// rows, m row-major 3 x 4): coefficients pl, |coefficient| row sums plm, |offset| sums pld.
struct FrustumPlanes {
    float pl[5][4], plm[5][3], pld[5];
};
RTR_HD FrustumPlanes frustum_planes(const float m[12], float fW, float fH) {
    FrustumPlanes f;
    const float comb[5][3] = {{0.f, 0.f, 1.f}, {1.f, 0.f, 1.f}, {-1.f, 0.f, fW}, {0.f, 1.f, 1.f}, {0.f, -1.f, fH}};
    for (int q = 0; q < 5; ++q) {
        for (int k = 0; k < 4; ++k) f.pl[q][k] = comb[q][0] * m[k] + comb[q][1] * m[4 + k] + comb[q][2] * m[8 + k];
        for (int k = 0; k < 3; ++k) f.plm[q][k] = __builtin_fabsf(comb[q][0] * m[k]) + __builtin_fabsf(comb[q][1] * m[4 + k]) + __builtin_fabsf(comb[q][2] * m[8 + k]);
        f.pld[q] = __builtin_fabsf(comb[q][0] * m[3]) + __builtin_fabsf(comb[q][1] * m[7]) + __builtin_fabsf(comb[q][2] * m[11]);
    }
    return f;
}
// The box [lo, hi] lies entirely on the wrong side of one half-space by more than 1e-4 x the magnitude of the terms
// involved: no point in it can pass the exact test (see "CULL" in rtr_kernels.hip).  NaN / inf boxes never do.
RTR_HD bool box_outside(const FrustumPlanes &f, const float lo[3], const float hi[3]) {
    bool culled = false;
    for (int q = 0; q < 5; ++q) {
        float v = f.pl[q][3], m = f.pld[q];
        for (int k = 0; k < 3; ++k) {
            const float t0 = f.pl[q][k] * lo[k], t1 = f.pl[q][k] * hi[k];
            v += t0 > t1 ? t0 : t1;
            const float e0 = __builtin_fabsf(lo[k]), e1 = __builtin_fabsf(hi[k]);
            m += f.plm[q][k] * (e0 > e1 ? e0 : e1);
        }
        culled = culled || (v < -1e-4f * m);
    }
    return culled;
}
// The box of a packed chunk from its header word {base x, base y, base z, widths} (rtr_kernels.h, PackedXyz).  An axis
// of b <= 25 bits has every value's bit pattern in [base, base | (2^b - 1)]; the sign bit is part of the common prefix,
// so the values lie between the floats of the two ends (swapped when the sign is negative; b = 0: one value).  Lanes
// past the cloud's end hold copies of its last quad, inside the box.  Returns false -- no box: keep the chunk -- for a
// wide chunk (some axis needs 32 bits: mixed signs, NaNs, -0 next to +0) or when an end is inf / NaN (base | mask can
// reach exponent 0xFF; the base then has a smaller one or the same).
RTR_HD bool chunk_box(uint32_t bx, uint32_t by, uint32_t bz, uint32_t widths, float lo[3], float hi[3]) {
    const uint32_t base[3] = {bx, by, bz};
    bool ok = (widths & kPackWideFlag) == 0u;
    for (int a = 0; a < 3; ++a) {
        const uint32_t b = (widths >> (6 * a)) & 31u;  // (<= 25 unless wide)
        const uint32_t top = base[a] | ((1u << b) - 1u);
        ok = ok && (top & 0x7F800000u) != 0x7F800000u;
        const float f0 = __builtin_bit_cast(float, base[a]), f1 = __builtin_bit_cast(float, top);
        const bool neg = (base[a] >> 31) != 0u;
        lo[a] = neg ? f1 : f0;
        hi[a] = neg ? f0 : f1;
    }
    return ok;
}

}  // namespace rtr
