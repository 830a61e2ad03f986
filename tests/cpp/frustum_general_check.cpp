// Host-side soundness check of the conservative rejections between the cloud and the exact projection, under general
// projection matrices (tests/camera_cases.py), built with g++ -ffp-contract=off and linked against the oracle's shared
// library.  argv[1] is a file of records written by tests/test_frustum_general.py:
//   int32 {matrix, pose, W, H, kind (0 straddle, 1 scene, 2 lanes), n, chunks}, float P[16], float xyz[n][3],
//   float box[chunks][6] (the exact min / max of each 256-point chunk: what k_chunk_bounds gives option "cull").
// For every record, with keep(p) = the oracle's orc_project_point puts p on a pixel:
//   1. box test: no box that rtr::box_outside(rtr::frustum_planes(P, W, H)) rejects holds a kept point -- over the
//      exact boxes and over the boxes rtr::chunk_box gives from the packed headers of the same chunks (pack_header: the
//      packer's common-prefix rule, the wide flag and the box word of a chunk that straddles a coordinate plane);
//   2. rectangle test: the same for rtr::rect_planes of random rectangles and the points that land inside them;
//   3. lane test (kinds 0 and 2): with s the chunk's measured lane spread (k_chunk_bounds' rule) and the constants
//      rtr::lane_test_consts gives from the cloud's absmax, no lane is rejected by the front step or the margin step
//      when the oracle keeps one of its four points;
//   4. quad test: no point that the oracle keeps is rejected by the per-point conservative test.
// 3. and 4. restate the device's predicates (a model: tests/test_gpu_general_cameras.py pins the kernel's own lines).
// Then 5.: 1. and 2. over 20 000 random matrices whose twelve entries draw their magnitudes independently from
// 1e-12 .. 1e12, boxes placed through the float64 inverse on and around each half-space.
// Prints one line per matrix "<matrix> <boxes> <rejected> <kept points> <rect rejections> <lanes> <lanes rejected>",
// a line "random <matrices> <boxes> <rejected> <kept points>", then "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "rtr_chunk_box.h"
#include "rtr_lane_test.h"

extern "C" int64_t orc_project_point(const float P[16], float x, float y, float z, int W, int H, uint32_t *depth_bits);

static uint32_t as_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static bool finite_bits(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }

// what k_pack_measure writes for a chunk of 256 patterns per axis, all of them points (tests/cpp/wide_box_check.cpp)
struct Header {
    uint32_t base[3], widths, wbox;
};
static Header pack_header(const uint32_t v[3][256]) {
    Header h{};
    int first_wide = -1;
    uint32_t w[3];
    bool all_finite = true;
    for (int a = 0; a < 3; ++a) {
        uint32_t diff = 0;
        for (int i = 0; i < 256; ++i) diff |= v[a][i] ^ v[a][0], all_finite = all_finite && finite_bits(v[a][i]);
        const uint32_t nb = diff ? 32u - (uint32_t)__builtin_clz(diff) : 0u;
        w[a] = nb > 25u ? 32u : nb;
        h.base[a] = w[a] == 32u ? 0u : (v[a][0] >> w[a]) << w[a];
        if (w[a] == 32u && first_wide < 0) first_wide = a;
    }
    h.widths = w[0] | (w[1] << 6) | (w[2] << 12) | (first_wide >= 0 ? rtr::kPackWideFlag : 0u);
    if (first_wide >= 0 && all_finite) {
        uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
        for (int i = 0; i < 256; ++i) {
            const uint32_t k = rtr::float_order_key(v[first_wide][i]);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
        h.wbox = rtr::wide_box_word(rtr::float_order_bits(kmin), rtr::float_order_bits(kmax));
    }
    return h;
}

// The rows as the point kernel computes them (project_rows / lane_maybe / do_quad in rtr_kernels.hip: the contract's
// arithmetic, one product, two fused multiply-adds and one sum per row)
static float row(const float *m, float x, float y, float z) { return std::fmaf(m[2], z, std::fmaf(m[1], y, m[0] * x)) + m[3]; }
static float min4(float a, float b, float c, float d) { return std::fmin(std::fmin(a, b), std::fmin(c, d)); }

// lane_maybe: the `front` line (the front step) and the `out` line (the margin step) of the light path
static bool lane_maybe(const float *P, const rtr::LaneTest &lt, float hiW, float hiH, float x0, float y0, float z0, float sp) {
    const float rz0 = row(P + 8, x0, y0, z0);
    const float sz = sp * lt.lz;
    const bool front = (rz0 + sz) > -lt.zfront;
    if (!front) return false;
    const float rx0 = row(P, x0, y0, z0), ry0 = row(P + 4, x0, y0, z0);
    const float m = min4(std::fmaf(hiW, rz0, -rx0), std::fmaf(hiH, rz0, -ry0), std::fmaf(0.75f, rz0, rx0), std::fmaf(0.75f, rz0, ry0));
    const bool out = ((rz0 - sz) > lt.zsafe) && (m < -(sp * lt.lall));
    return !out;
}
// do_quad: `front` (r.z > 0) and the quad test `z > 1e-30f && m < 0`
static bool quad_maybe(const float *P, float hiW, float hiH, float x, float y, float z) {
    const float rz = row(P + 8, x, y, z), rx = row(P, x, y, z), ry = row(P + 4, x, y, z);
    const float m = min4(std::fmaf(hiW, rz, -rx), std::fmaf(hiH, rz, -ry), std::fmaf(0.75f, rz, rx), std::fmaf(0.75f, rz, ry));
    const bool out = (rz > 1e-30f) && (m < 0.0f);
    return (rz > 0.0f) && !out;
}

struct Counts {
    long boxes = 0, rejected = 0, kept = 0, rect_rejected = 0, lanes = 0, lanes_rejected = 0;
};

static int fail(const char *what, int matrix, int pose, int W, int H, int kind, long chunk, const float *p) {
    std::printf("FAIL %s: matrix %d pose %d %dx%d kind %d chunk %ld point (%a %a %a)\n", what, matrix, pose, W, H, kind, chunk, p[0], p[1], p[2]);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::mt19937_64 rng(0xCA3E7Aull);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    std::vector<Counts> per;
    int32_t hd[7];
    while (std::fread(hd, 4, 7, in) == 7) {
        const int matrix = hd[0], pose = hd[1], W = hd[2], H = hd[3], kind = hd[4];
        const long n = hd[5], chunks = hd[6];
        float P[16];
        std::vector<float> xyz(3 * (size_t)n), box(6 * (size_t)chunks);
        if (std::fread(P, 4, 16, in) != 16 || std::fread(xyz.data(), 4, xyz.size(), in) != xyz.size() ||
            std::fread(box.data(), 4, box.size(), in) != box.size() || chunks != (n + 255) / 256)
            return 2;
        if ((size_t)matrix >= per.size()) per.resize(matrix + 1);
        Counts &cnt = per[matrix];
        std::vector<int64_t> pix(n);
        float absmax[3] = {0.f, 0.f, 0.f};
        for (long i = 0; i < n; ++i) {
            pix[i] = orc_project_point(P, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], W, H, nullptr);
            cnt.kept += pix[i] >= 0;
            for (int a = 0; a < 3; ++a) absmax[a] = std::fmax(absmax[a], std::fabs(xyz[3 * i + a]));
        }
        const rtr::FrustumPlanes fp = rtr::frustum_planes(P, (float)W, (float)H);
        // the rectangles of this record: random, thin, on the borders, the whole frame
        const int nrect = kind == 2 ? 0 : 16;
        int rc[16][4];
        rtr::FrustumPlanes rp[16];
        for (int r = 0; r < nrect; ++r) {
            int x0 = (int)(rng() % W), x1 = (int)(rng() % W), y0 = (int)(rng() % H), y1 = (int)(rng() % H);
            if (x0 > x1) std::swap(x0, x1);
            if (y0 > y1) std::swap(y0, y1);
            ++x1, ++y1;
            if (r % 8 == 1) x1 = x0 + 1;
            if (r % 8 == 2) y1 = y0 + 1;
            if (r % 8 == 3) x0 = 0, y0 = 0;
            if (r % 8 == 4) x1 = W, y1 = H;
            if (r % 8 == 5) x0 = 0, y0 = 0, x1 = W, y1 = H;
            rc[r][0] = x0, rc[r][1] = y0, rc[r][2] = x1, rc[r][3] = y1;
            rp[r] = rtr::rect_planes(P, (float)x0, (float)y0, (float)x1, (float)y1);
        }
        const rtr::LaneTest lt = rtr::lane_test_consts(P, W, H, absmax);
        const float hiW = (float)W + 0.25f, hiH = (float)H + 0.25f;
        for (long c = 0; c < chunks; ++c) {
            // the chunk's points; past the cloud's end copies of the last one (inside every box)
            float p[256][3];
            uint32_t v[3][256];
            int64_t px[256];
            bool any = false;
            for (int i = 0; i < 256; ++i) {
                const long j = 256 * c + i < n ? 256 * c + i : n - 1;
                for (int a = 0; a < 3; ++a) p[i][a] = xyz[3 * j + a], v[a][i] = as_bits(p[i][a]);
                px[i] = pix[j];
                any = any || px[i] >= 0;
            }
            float lo[2][3], hi[2][3];
            bool have[2] = {true, false};
            for (int a = 0; a < 3; ++a) lo[0][a] = box[6 * c + a], hi[0][a] = box[6 * c + 3 + a];
            const Header h = pack_header(v);
            have[1] = rtr::chunk_box(h.base[0], h.base[1], h.base[2], h.widths, h.wbox, lo[1], hi[1]);
            for (int b = 0; b < 2; ++b) {
                if (!have[b]) continue;
                for (int i = 0; i < 256; ++i)
                    for (int a = 0; a < 3; ++a)
                        if (!(p[i][a] >= lo[b][a] && p[i][a] <= hi[b][a])) return fail(b ? "packed box does not hold the point" : "box does not hold the point", matrix, pose, W, H, kind, c, p[i]);
                ++cnt.boxes;
                const bool rej = rtr::box_outside(fp, lo[b], hi[b]);
                cnt.rejected += rej;
                if (rej && any)
                    for (int i = 0; i < 256; ++i)
                        if (px[i] >= 0) return fail(b ? "packed box rejected" : "box rejected", matrix, pose, W, H, kind, c, p[i]);
                for (int r = 0; r < nrect; ++r) {
                    if (!rtr::box_outside(rp[r], lo[b], hi[b])) continue;
                    ++cnt.rect_rejected;
                    for (int i = 0; i < 256 && any; ++i) {
                        const int x = (int)(px[i] % W), y = (int)(px[i] / W);
                        if (px[i] >= 0 && x >= rc[r][0] && x < rc[r][2] && y >= rc[r][1] && y < rc[r][3])
                            return fail(b ? "packed box rejected for a rectangle" : "box rejected for a rectangle", matrix, pose, W, H, kind, c, p[i]);
                    }
                }
            }
            // the quad test, point by point
            for (int i = 0; i < 256; ++i)
                if (px[i] >= 0 && !quad_maybe(P, hiW, hiH, p[i][0], p[i][1], p[i][2])) return fail("quad test rejected", matrix, pose, W, H, kind, c, p[i]);
            if (kind == 1) continue;
            // the lane test: the spread as k_chunk_bounds measures it (one rounding per difference, then x 1.000001)
            float sp = 0.f;
            for (int l = 0; l < 64; ++l)
                for (int k = 1; k < 4; ++k)
                    for (int a = 0; a < 3; ++a) sp = std::fmax(sp, std::fabs(p[4 * l + k][a] - p[4 * l][a]));
            sp *= 1.000001f;
            for (int l = 0; l < 64; ++l) {
                const bool cand = lane_maybe(P, lt, hiW, hiH, p[4 * l][0], p[4 * l][1], p[4 * l][2], sp);
                ++cnt.lanes;
                cnt.lanes_rejected += !cand;
                for (int k = 0; k < 4 && !cand; ++k)
                    if (px[4 * l + k] >= 0) return fail("lane test rejected", matrix, pose, W, H, kind, c, p[4 * l + k]);
            }
        }
    }
    std::fclose(in);
    for (size_t m = 0; m < per.size(); ++m)
        std::printf("%zu %ld %ld %ld %ld %ld %ld\n", m, per[m].boxes, per[m].rejected, per[m].kept, per[m].rect_rejected, per[m].lanes, per[m].lanes_rejected);

    // 5. random matrices
    long rmat = 0, rboxes = 0, rrej = 0, rkept = 0;
    for (int t = 0; t < 20000; ++t) {
        float P[16] = {0};
        double M[3][4];
        for (int k = 0; k < 12; ++k) {
            const double mag = std::pow(10.0, -12.0 + 24.0 * u01(rng));
            P[k] = (float)((rng() & 1) ? -mag : mag);
            M[k / 4][k % 4] = (double)P[k];
        }
        P[15] = 1.f;
        const int W = (rng() & 1) ? 160 : 1920, H = W == 160 ? 128 : 1080;
        // the float64 inverse of the 3 x 3 part (adjugate / determinant) and the camera centre
        double adj[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                adj[j][i] = M[(i + 1) % 3][(j + 1) % 3] * M[(i + 2) % 3][(j + 2) % 3] - M[(i + 1) % 3][(j + 2) % 3] * M[(i + 2) % 3][(j + 1) % 3];
        const double det = M[0][0] * adj[0][0] + M[0][1] * adj[1][0] + M[0][2] * adj[2][0];
        if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) continue;
        ++rmat;
        auto back = [&](const double r[3], double out[3]) {  // M^-1 (r - t)
            for (int i = 0; i < 3; ++i) out[i] = (adj[i][0] * (r[0] - M[0][3]) + adj[i][1] * (r[1] - M[1][3]) + adj[i][2] * (r[2] - M[2][3])) / det;
        };
        const rtr::FrustumPlanes fp = rtr::frustum_planes(P, (float)W, (float)H);
        int x0 = (int)(rng() % W), x1 = (int)(rng() % W), y0 = (int)(rng() % H), y1 = (int)(rng() % H);
        if (x0 > x1) std::swap(x0, x1);
        if (y0 > y1) std::swap(y0, y1);
        ++x1, ++y1;
        const rtr::FrustumPlanes rp = rtr::rect_planes(P, (float)x0, (float)y0, (float)x1, (float)y1);
        // the scale of r.z: what the matrix gives points about as far from the centre as the centre is from the origin
        const double zt = std::fabs(M[2][3]) > 0 ? std::fabs(M[2][3]) : 1.0;
        for (int b = 0; b < 12; ++b) {
            const int q = b % 6;  // 0: the camera plane, 1..4: a side, 5: inside
            const double d = zt * std::pow(10.0, -3.0 + 6.0 * u01(rng));
            double u = W * u01(rng), v = H * u01(rng), z = d;
            const double off = (b < 6) ? 0.0 : 3.0 * (u01(rng) - 0.5);  // on the plane, or up to 1.5 px beside it
            if (q == 0) z = d * 1e-3 * (u01(rng) - 0.5);
            if (q == 1) u = -0.5 + off;
            if (q == 2) u = W - 0.5 + off;
            if (q == 3) v = -0.5 + off;
            if (q == 4) v = H - 0.5 + off;
            const double r[3] = {u * z, v * z, z};
            double ctr[3];
            back(r, ctr);
            float lo[3], hi[3];
            const double size = std::pow(10.0, -7.0 + 6.0 * u01(rng));
            bool ok = true;
            for (int a = 0; a < 3; ++a) {
                const double e = std::fabs(ctr[a]) * size * u01(rng);
                lo[a] = (float)(ctr[a] - e), hi[a] = (float)(ctr[a] + e);
                ok = ok && std::isfinite(lo[a]) && std::isfinite(hi[a]);
            }
            if (!ok) continue;
            ++rboxes;
            const bool rej = rtr::box_outside(fp, lo, hi), rrect = rtr::box_outside(rp, lo, hi);
            rrej += rej;
            for (int s = 0; s < 8 + 24; ++s) {
                float p[3];
                for (int a = 0; a < 3; ++a) {
                    if (s < 8) p[a] = ((s >> a) & 1) ? hi[a] : lo[a];
                    else {
                        p[a] = (float)((double)lo[a] + ((double)hi[a] - (double)lo[a]) * u01(rng));
                        p[a] = p[a] < lo[a] ? lo[a] : (p[a] > hi[a] ? hi[a] : p[a]);
                    }
                }
                const int64_t px = orc_project_point(P, p[0], p[1], p[2], W, H, nullptr);
                rkept += px >= 0;
                if (px >= 0 && rej) return fail("random matrix: box rejected", t, 0, W, H, q, b, p);
                if (px >= 0 && rrect && px % W >= x0 && px % W < x1 && px / W >= y0 && px / W < y1)
                    return fail("random matrix: box rejected for a rectangle", t, 0, W, H, q, b, p);
                if (px >= 0 && !quad_maybe(P, (float)W + 0.25f, (float)H + 0.25f, p[0], p[1], p[2])) return fail("random matrix: quad test rejected", t, 0, W, H, q, b, p);
            }
        }
    }
    std::printf("random %ld %ld %ld %ld\nok\n", rmat, rboxes, rrej, rkept);
    return 0;
}
