/* point_pass_ref.c -- the reference answer of rtr_point_pass (include/rtr.h section 6b), from the oracle's
 * projection: built by tests/point_pass_ref.py with the system C compiler and linked against oracle/librtr_oracle.so.
 * A whole-cloud loop in C, so 1e7 points take about a second.
 *   xyz: n points, xyz_stride bytes apart (x, y, z fp32); depth: the frame's depth bits [W*H];
 *   ids [W*H]: smallest upload index whose depth bits are the pixel's, 0xFFFFFFFF for none;
 *   vis [(n + 31) / 32]: bit i % 32 of word i / 32 = point i projects and !(d > depth[pix] + window). */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

int64_t orc_project_point(const float P[16], float x, float y, float z, int W, int H, uint32_t *depth_bits);

void ppr_point_pass(const void *xyz, size_t xyz_stride, size_t n, const float P[16], int W, int H, const uint32_t *depth,
                    float window, uint32_t *ids, uint32_t *vis) {
    const size_t npix = (size_t)W * H;
    for (size_t p = 0; p < npix; ++p) ids[p] = 0xFFFFFFFFu;
    memset(vis, 0, ((n + 31) / 32) * sizeof(uint32_t));
    for (size_t i = 0; i < n; ++i) {
        const float *q = (const float *)((const char *)xyz + i * xyz_stride);
        uint32_t bits = 0;
        const int64_t pix = orc_project_point(P, q[0], q[1], q[2], W, H, &bits);
        if (pix < 0) continue;
        const uint32_t m = depth[pix];
        if (bits == m && (uint32_t)i < ids[pix]) ids[pix] = (uint32_t)i;
        float d, md;
        memcpy(&d, &bits, 4);
        memcpy(&md, &m, 4);
        const float lim = md + window; /* one fp32 add: built with -ffp-contract=off */
        if (!(d > lim)) vis[i / 32] |= 1u << (i % 32);
    }
}
