/* ref_driver.cpp -- runs the reference's kernels, compiled for the host, one call per CUDA thread (test infrastructure).
 *
 * oracle/ref_build.py links this file with two translation units made of the reference's own, unchanged text
 * (src/render.cu, and the kernel region of src/project_cloud.cu) into oracle/_ref/libref_<variant>.so.  Nothing of the
 * reference is restated here except its LAUNCH code -- which kernel, in which order, with which grid, block, buffers
 * and sizes -- because that is host code bound to the CUDA runtime, OpenCV and torch.  Every such line cites the
 * reference line it follows (paths under src/RTRenderer/; `pc:` = src/project_cloud.cu, `r:` = src/render.cu).
 *
 * How a launch is run.  `kernel<<<grid, block>>>(args)` becomes: for every block index, for every thread index, set
 * gridDim / blockDim / blockIdx / threadIdx (cuda_shim.h) and call kernel(args).  The kernels of this path are
 * thread-independent apart from (a) the warp votes of minDepthPass / accumulatePass, run as a warp with one active
 * lane (cuda_shim.h), and (b) the shared-memory trees of the two min/max kernels, which are launched with
 * blockDim.x = 1 instead of `block_size`: the stride loop then does all the work and the tree loop never runs -- a
 * legal launch of the same text with the same result (min and max of the same elements).
 *
 * block_size (pc:216) comes from cudaOccupancyMaxPotentialBlockSize on the reference's GPU; it only splits the index
 * range into blocks, so the result does not depend on it (tests run 1024 and another value).  Memory that cudaMalloc
 * leaves undefined is filled with a caller-chosen POISON byte, so that a test can see which elements no kernel wrote.
 * Buffers get `slack` extra elements (default 1): resolvePass tests `id > count` (r:145), not `id >= count`.
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cuda_shim.h"
#include "filter_prelude.h"
#include "render.cuh" /* the reference's own declarations of the render.cu kernels (-I <reference>/include) */

/* the five kernels of the cut region of project_cloud.cu (pc:28-187): their signatures, cut out next to it by ref_build.py */
#include "project_cloud_kernels.h"

__thread dim3 blockIdx, blockDim, threadIdx, gridDim;
/* the `extern __shared__` arrays of r:169 and r:209: 2 * blockDim.x words, blockDim.x = 1 */
uint32_t s_min_max[2], s_min_max_final[2];

namespace {

int g_block_size = 1024; /* pc:216 */
int g_slack = 1;
int g_poison = 0xA5;

template <class Call> void launch(dim3 grid, dim3 block, Call call) {
    gridDim = grid;
    blockDim = block;
    for (unsigned bz = 0; bz < grid.z; ++bz)
        for (unsigned by = 0; by < grid.y; ++by)
            for (unsigned bx = 0; bx < grid.x; ++bx)
                for (unsigned tz = 0; tz < block.z; ++tz)
                    for (unsigned ty = 0; ty < block.y; ++ty)
                        for (unsigned tx = 0; tx < block.x; ++tx) {
                            blockIdx.x = bx; blockIdx.y = by; blockIdx.z = bz;
                            threadIdx.x = tx; threadIdx.y = ty; threadIdx.z = tz;
                            call();
                        }
}
dim3 d1(unsigned x) { return dim3{x, 1, 1}; }

template <class T> struct DeviceBuffer { /* cudaMalloc: `count` elements of undefined (poisoned) memory, plus slack */
    std::vector<T> v;
    void alloc(size_t count) {
        v.assign(count + (size_t)g_slack, T());
        if (!v.empty()) std::memset(static_cast<void *>(v.data()), g_poison, v.size() * sizeof(T));
    }
    T *ptr() { return v.data(); }
};

struct Renderer {
    int W = 0, H = 0;
    size_t data_size = 0;
    int block_size = 1024, numBlocksPCDLevel = 0, numBlocksImgLevel = 0;
    dim3 block_dim{16, 16, 1}, grid_dim{1, 1, 1};
    uint2 image_size{1, 1};
    DeviceBuffer<float4> d_vertices_data;
    DeviceBuffer<uchar4> d_color_data;
    DeviceBuffer<uint32_t> d_output_color, d_output_depth, d_local_mins, d_local_maxes, d_final_min, d_final_max;
    DeviceBuffer<uint8_t> d_image;
    DeviceBuffer<c10::Half> tensorPtr;
    float d_cam_proj[16];
    std::vector<uint8_t> last_mask; /* a host copy of the level-0 mask, taken before pc:390 frees it */
    int mask_w = 0, mask_h = 0;

    /* pc:189-217 (constructor) and pc:275-298 (the resize branch of every compute* entry point) */
    void setup(const float *xyzw, const uint8_t *rgba, size_t n, const float *P, int width, int height) {
        W = width; H = height; data_size = n;
        block_size = g_block_size;
        block_dim.x = 16; block_dim.y = 16; block_dim.z = 1;                                   /* pc:196-198 */
        d_vertices_data.alloc(n); d_color_data.alloc(n);                                        /* pc:200-201 */
        if (n) { std::memcpy(d_vertices_data.ptr(), xyzw, n * sizeof(float4)); std::memcpy(d_color_data.ptr(), rgba, n * sizeof(uchar4)); }
        d_final_max.alloc(1); d_final_min.alloc(1);                                             /* pc:203-204 */
        numBlocksPCDLevel = (int)((data_size + block_size - 1) / block_size);                   /* pc:217 */
        numBlocksImgLevel = (W * H + block_size - 1) / block_size;                              /* pc:284 */
        d_local_maxes.alloc(numBlocksImgLevel); d_local_mins.alloc(numBlocksImgLevel);          /* pc:285-286 */
        d_output_color.alloc((size_t)W * H * 4);                                                /* pc:288 */
        d_image.alloc((size_t)W * H * 3);                                                       /* pc:289 */
        d_output_depth.alloc((size_t)W * H);                                                    /* pc:290 */
        tensorPtr.alloc((size_t)W * H * 5);                                                     /* pc:291 */
        grid_dim.x = W / block_dim.x; grid_dim.y = H / block_dim.y; grid_dim.z = 1;             /* pc:293-295 */
        image_size = uint2{static_cast<unsigned int>(W), static_cast<unsigned int>(H)};         /* pc:297 */
        if (P) std::memcpy(d_cam_proj, P, sizeof d_cam_proj); /* pc:318-320: the composed matrix, row-major, is an input */
    }

    /* pc:314-329 computeRGBDInternal */
    void computeRGBDInternal() {
        uint32_t *depth = d_output_depth.ptr(), *color = d_output_color.ptr();
        const float4 *vertices = d_vertices_data.ptr();
        const uchar4 *colors = d_color_data.ptr();
        uint8_t *image = d_image.ptr();
        const float *cam_proj = d_cam_proj;
        launch(grid_dim, block_dim, [&] { fillBuffer(depth, 0x7F7FFFFF, W * H); });                              /* pc:316 */
        std::memset(color, 0, (size_t)W * H * 4 * sizeof(uint32_t));                                             /* pc:317 */
        launch(d1(numBlocksPCDLevel), d1(block_size), [&] { minDepthPass(depth, vertices, cam_proj, image_size, data_size); });          /* pc:321 */
        launch(d1(numBlocksPCDLevel), d1(block_size), [&] { accumulatePass(vertices, colors, data_size, image_size, cam_proj, depth, color); }); /* pc:323 */
        launch(grid_dim, block_dim, [&] { resolvePass(image, color, W * H); });                                  /* pc:325 */
    }

    /* pc:331-392 applyDepthFilter; depthRescaleDepth = 4 (pc:23) */
    void applyDepthFilter() {
        const int depthRescaleDepth = 4;
        std::vector<DeviceBuffer<float>> owned(depthRescaleDepth + 1);
        std::vector<float *> imgResolutions(depthRescaleDepth + 1);                                              /* pc:333 */
        imgResolutions[0] = reinterpret_cast<float *>(d_output_depth.ptr());                                     /* pc:334 */
        int newWidth = W, newHeight = H;                                                                         /* pc:336-337 */
        int nrBlocks = (int)((newWidth * newHeight + block_size - 1) / block_size);                              /* pc:338 */
        for (size_t i = 1; i < imgResolutions.size(); ++i) {                                                     /* pc:340 */
            newWidth /= 2; newHeight /= 2;                                                                       /* pc:342-343 */
            nrBlocks = (int)((newWidth * newHeight + block_size - 1) / block_size);                              /* pc:344 */
            owned[i].alloc((size_t)newWidth * newHeight);                                                        /* pc:346 */
            imgResolutions[i] = owned[i].ptr();
            float *hi = imgResolutions[i - 1], *lo = imgResolutions[i];
            launch(d1(nrBlocks), d1(block_size), [&] { reduce(hi, lo, newWidth, newHeight); });                  /* pc:348 */
        }
        for (int i = (int)imgResolutions.size() - 1; i >= 1; --i) {                                              /* pc:352 */
            DeviceBuffer<uint8_t> gradMaskBuf;
            gradMaskBuf.alloc((size_t)newWidth * newHeight);                                                     /* pc:355 */
            uint8_t *gradMask = gradMaskBuf.ptr();
            float *cur = imgResolutions[i], *finer = imgResolutions[i - 1];
            launch(d1(nrBlocks), d1(block_size), [&] { laplacianKernel(cur, gradMask, newWidth, newHeight); });  /* pc:357 */
            newWidth *= 2; newHeight *= 2;                                                                       /* pc:360-361 */
            nrBlocks = (int)((newWidth * newHeight + block_size - 1) / block_size);                              /* pc:362 */
            DeviceBuffer<uint8_t> maskBuf;
            maskBuf.alloc((size_t)newWidth * newHeight);                                                         /* pc:365 */
            uint8_t *mask = maskBuf.ptr();
            launch(d1(nrBlocks), d1(block_size), [&] { compareImgsKernel(cur, finer, gradMask, mask, newWidth, newHeight); }); /* pc:367 */
            if (i == 1) {                                                                                        /* pc:372 */
                uint32_t *mins = d_local_mins.ptr(), *maxes = d_local_maxes.ptr();
                uint32_t *fmin = d_final_min.ptr(), *fmax = d_final_max.ptr();
                uint32_t *depth = d_output_depth.ptr();
                /* pc:375, pc:377 with blockDim.x = 1 (see the head of this file) */
                launch(d1(nrBlocks), d1(1), [&] { find_local_minmax_kernel(depth, mins, maxes, newWidth * newHeight); });
                launch(d1(1), d1(1), [&] { find_overall_minmax_kernel(mins, maxes, fmin, fmax, nrBlocks); });
                uint8_t *image = d_image.ptr();
                c10::Half *tensor = tensorPtr.ptr();
                launch(d1(nrBlocks), d1(block_size), [&] { removeMask(finer, image, mask, tensor, fmin, fmax, newWidth, newHeight); }); /* pc:380 */
                last_mask.assign(mask, mask + (size_t)newWidth * newHeight);
                mask_w = newWidth; mask_h = newHeight;
            } else {
                launch(d1(nrBlocks), d1(block_size), [&] { resizeKernel(cur, finer, mask, newWidth, newHeight); }); /* pc:385 */
            }
        }
    }

    void copy_unfiltered(uint32_t *depth, uint32_t *acc, uint8_t *img) {
        const size_t npix = (size_t)W * H;
        if (depth) std::memcpy(depth, d_output_depth.ptr(), npix * 4);
        if (acc) std::memcpy(acc, d_output_color.ptr(), npix * 16);
        if (img) std::memcpy(img, d_image.ptr(), npix * 3);
    }
    void copy_filtered(uint32_t *depth, uint8_t *img, uint8_t *mask, int *mask_dims, uint32_t *minmax, uint16_t *tensor) {
        const size_t npix = (size_t)W * H;
        if (depth) std::memcpy(depth, d_output_depth.ptr(), npix * 4);
        if (img) std::memcpy(img, d_image.ptr(), npix * 3);
        if (mask) std::memcpy(mask, last_mask.data(), last_mask.size());
        if (mask_dims) { mask_dims[0] = mask_w; mask_dims[1] = mask_h; }
        if (minmax) { minmax[0] = *d_final_min.ptr(); minmax[1] = *d_final_max.ptr(); }
        if (tensor) std::memcpy(tensor, static_cast<void *>(tensorPtr.ptr()), npix * 5 * sizeof(uint16_t));
    }
};

bool bad_dims(int W, int H) { return W <= 0 || H <= 0 || (long long)W * H > (1ll << 26); }

}  // namespace

extern "C" {

int ref_abi(void) { return 1; }

/* What this build's flags do to `a * b + c` and to __fdividef: bit 0 set = the compiler contracted the expression into
 * one fma, bit 1 set = IEEE division (REF_FDIVIDEF_IEEE).  The tests check it against the variant's name. */
int ref_build_traits(void) {
    volatile float a = 1.0f + 0x1p-12f, b = 1.0f + 0x1p-12f, c = -(1.0f + 0x1p-11f);
    const float x = a, y = b, z = c;
    const float r = x * y + z; /* 0 with two roundings, 2^-24 fused */
    int traits = (r != 0.0f) ? 1 : 0;
    volatile float p = 5.0f, q = 3.0f; /* 5 / 3 and 5 * RN(1/3) differ in the last bit */
    const float ieee = p / q;
    if (__float_as_uint(__fdividef(p, q)) == __float_as_uint(ieee)) traits |= 2;
    return traits;
}

/* block_size: pc:216; slack: extra elements behind every device buffer; poison: the byte undefined memory holds */
void ref_config(int block_size, int slack, int poison) {
    g_block_size = block_size > 0 ? block_size : 1024;
    g_slack = slack < 0 ? 0 : slack;
    g_poison = poison & 0xFF;
}

/* computeRGBD without the filter (pc:268-312): xyzw float4[n], rgba uchar4[n], P row-major float[16].
 * -> depth u32[W*H] (float bits), acc u32[W*H*4], img u8[W*H*3]; elements no kernel wrote hold the poison byte. */
int ref_project(const float *xyzw, const uint8_t *rgba, size_t n, const float *P, int W, int H, uint32_t *depth,
                uint32_t *acc, uint8_t *img) {
    if (bad_dims(W, H)) return -1;
    Renderer r;
    r.setup(xyzw, rgba, n, P, W, H);
    r.computeRGBDInternal();
    r.copy_unfiltered(depth, acc, img);
    return 0;
}

/* applyDepthFilter (pc:331-392) on a GIVEN unfiltered frame: depth u32[W*H] and img u8[W*H*3] are in/out.
 * mask: u8[W*H], the first mask_dims[0] * mask_dims[1] bytes are the level-0 mask (row stride mask_dims[0]);
 * minmax u32[2]; tensor: fp16 bits [5*W*H] exactly as the reference lays them out (plane stride
 * mask_dims[0] * mask_dims[1]; the rest holds the poison byte). */
int ref_filter(uint32_t *depth, uint8_t *img, int W, int H, uint8_t *mask, int *mask_dims, uint32_t *minmax,
               uint16_t *tensor) {
    if (bad_dims(W, H) || (H >> 4) < 1 || (W >> 4) < 1) return -1;
    Renderer r;
    r.setup(nullptr, nullptr, 0, nullptr, W, H);
    std::memcpy(r.d_output_depth.ptr(), depth, (size_t)W * H * 4);
    std::memcpy(r.d_image.ptr(), img, (size_t)W * H * 3);
    r.applyDepthFilter();
    r.copy_filtered(depth, img, mask, mask_dims, minmax, tensor);
    return 0;
}

/* One launch of resizeKernel as at pc:385, on given levels: lo float[(outW/2)*(outH/2)], hi float[outW*outH] in/out,
 * mask u8[outW*outH].  The blended values reach a frame's outputs only through comparisons; this shows them. */
int ref_resize(const float *lo, float *hi, const uint8_t *mask, int outW, int outH) {
    if (bad_dims(outW, outH) || outW < 2 || outH < 2) return -1;
    const int nrBlocks = (int)((outW * outH + g_block_size - 1) / g_block_size);                                 /* pc:362 */
    DeviceBuffer<float> dlo, dhi;
    DeviceBuffer<uint8_t> dmask;
    dlo.alloc((size_t)(outW / 2) * (outH / 2)); dhi.alloc((size_t)outW * outH); dmask.alloc((size_t)outW * outH);
    std::memcpy(dlo.ptr(), lo, (size_t)(outW / 2) * (outH / 2) * 4);
    std::memcpy(dhi.ptr(), hi, (size_t)outW * outH * 4);
    std::memcpy(dmask.ptr(), mask, (size_t)outW * outH);
    float *l = dlo.ptr(), *h = dhi.ptr();
    uint8_t *m = dmask.ptr();
    launch(d1(nrBlocks), d1(g_block_size), [&] { resizeKernel(l, h, m, outW, outH); });                          /* pc:385 */
    std::memcpy(hi, dhi.ptr(), (size_t)outW * outH * 4);
    return 0;
}

/* computeFilteredRGBD (pc:394-434): both stages on one set of buffers; the unfiltered frame is copied out in between. */
int ref_frame(const float *xyzw, const uint8_t *rgba, size_t n, const float *P, int W, int H, uint32_t *depth_unf,
              uint32_t *acc, uint8_t *img_unf, uint32_t *depth, uint8_t *img, uint8_t *mask, int *mask_dims,
              uint32_t *minmax, uint16_t *tensor) {
    if (bad_dims(W, H) || (H >> 4) < 1 || (W >> 4) < 1) return -1;
    Renderer r;
    r.setup(xyzw, rgba, n, P, W, H);
    r.computeRGBDInternal();                                                                                     /* pc:421 */
    r.copy_unfiltered(depth_unf, acc, img_unf);
    r.applyDepthFilter();                                                                                        /* pc:422 */
    r.copy_filtered(depth, img, mask, mask_dims, minmax, tensor);
    return 0;
}

}  // extern "C"

#ifdef REF_HOST_MAIN
/* Stand-alone program for the sanitizers (CPU only): one 160x120 frame of a seeded cloud through ref_frame.
 *   ref_check [slack] [block_size]     prints one checksum per output; slack 0 runs the buffers at their exact size.
 * 120 % 16 != 0, so the tail rows that the reference's grids never write are part of the run. */
static uint64_t fnv(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
int main(int argc, char **argv) {
    const int slack = argc > 1 ? std::atoi(argv[1]) : 1, bs = argc > 2 ? std::atoi(argv[2]) : 1024;
    ref_config(bs, slack, 0xA5);
    const int W = 160, H = 120;
    const size_t n = 30000;
    std::vector<float> xyzw(4 * n);
    std::vector<uint8_t> rgba(4 * n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto u01 = [&s] { s = s * 6364136223846793005ull + 1442695040888963407ull; return (float)(s >> 40) * 0x1p-24f; };
    for (size_t i = 0; i < n; ++i) {
        xyzw[4 * i + 0] = -3.0f + 6.0f * u01();
        xyzw[4 * i + 1] = -2.0f + 4.0f * u01();
        xyzw[4 * i + 2] = -0.5f + 5.0f * u01(); /* some points behind the camera */
        xyzw[4 * i + 3] = 1.0f;
        for (int k = 0; k < 4; ++k) rgba[4 * i + k] = (uint8_t)(u01() * 256.0f);
    }
    const float P[16] = {160, 0, 80, 0, 0, 160, 60, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const size_t npix = (size_t)W * H;
    std::vector<uint32_t> du(npix), acc(4 * npix), d(npix), mm(2);
    std::vector<uint8_t> iu(3 * npix), im(3 * npix), mask(npix);
    std::vector<uint16_t> tensor(5 * npix);
    int dims[2] = {0, 0};
    if (ref_frame(xyzw.data(), rgba.data(), n, P, W, H, du.data(), acc.data(), iu.data(), d.data(), im.data(), mask.data(),
                  dims, mm.data(), tensor.data()) != 0) return 2;
    std::printf("unfiltered %016llx %016llx %016llx\n", (unsigned long long)fnv(du.data(), npix * 4),
                (unsigned long long)fnv(acc.data(), npix * 16), (unsigned long long)fnv(iu.data(), npix * 3));
    std::printf("filtered %016llx %016llx %016llx %016llx mask %dx%d minmax %08x %08x\n",
                (unsigned long long)fnv(d.data(), npix * 4), (unsigned long long)fnv(im.data(), npix * 3),
                (unsigned long long)fnv(mask.data(), (size_t)dims[0] * dims[1]), (unsigned long long)fnv(tensor.data(), npix * 10),
                dims[0], dims[1], mm[0], mm[1]);
    return 0;
}
#endif
