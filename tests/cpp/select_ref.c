/* Reference of the rectangle half of rtr_select_points (include/rtr.h section 6f) from the oracle's projection:
 * pix[i] = orc_project_point of point i (its pixel id, -1 when the frame does not accept it).  Built by
 * tests/select_ref.py with the system C compiler against the oracle's shared library. */
#include <stddef.h>
#include <stdint.h>

int64_t orc_project_point(const float P[16], float x, float y, float z, int W, int H, uint32_t *depth_bits);

void sref_pixels(const unsigned char *xyz, size_t stride, size_t n, const float P[16], int W, int H, int64_t *pix) {
    for (size_t i = 0; i < n; ++i) {
        const float *p = (const float *)(xyz + i * stride);
        pix[i] = orc_project_point(P, p[0], p[1], p[2], W, H, 0);
    }
}
