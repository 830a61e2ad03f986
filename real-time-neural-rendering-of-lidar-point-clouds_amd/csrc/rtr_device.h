// rtr_device.h -- device-side helpers shared by the kernel files (rtr_kernels.hip: the frame path, the upload, the
// point pass, extract and transform; rtr_cloud_kernels.hip: keep mask, remove, scan, select; rtr_voxel.hip and
// rtr_neighbours.hip, through rtr_key_sweep.h: the key sweeps of the voxel grid and the neighbour search;
// rtr_neighbours.hip, rtr_clusters.hip and rtr_near.hip: the pair test and the binary search in the sorted keys).
// Device-only: every function is __device__ __forceinline__, so no device call crosses a translation unit and no
// relocatable device code is needed.  Included by those files and nothing else; the arithmetic contract of
// rtr_kernels.hip (-ffp-contract=off) holds for all.
#pragma once
#include "rtr_kernels.h"

namespace rtr {

#define RTR_EMPTY 0x7F7FFFFFu
constexpr int kBlock = 256;   // 4 waves
// The grid-stride point kernels run Cloud::grid workgroups (kDefaultPointGrid = 1024, i.e. 4
// per CU, measured best: 1024 -> 205 us, 1536 -> 218, 2048 -> 239 for k_project_bin; 2048 would
// not even be co-resident: its 84 SGPRs admit 7 x 256 threads per CU, not 8).

// one rounding per operation: plain operators under -ffp-contract=off (hipcc's __fmul_rn &
// co. are the same plain operators; __fsqrt_rn is NOT correctly rounded, sqrtf is)
__device__ __forceinline__ float f_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float f_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f_sub(float a, float b) { return a - b; }

// the pair test of the radius searches (neighbours, clusters, near): the squared distance of (x, y, z) and (cx, cy, cz) as
// three differences, three products and two sums, each rounded on its own, in the order ((dx dx + dy dy) + dz dz)
__device__ __forceinline__ float pair_dist2(float x, float y, float z, float cx, float cy, float cz) {
    const float dx = f_sub(x, cx), dy = f_sub(y, cy), dz = f_sub(z, cz);
    return f_add(f_add(f_mul(dx, dx), f_mul(dy, dy)), f_mul(dz, dz));
}

// the first index in [0, m) of the sorted keys whose key is >= target (m: none)
__device__ __forceinline__ uint32_t key_lower_bound(const uint64_t *__restrict__ keys, uint32_t m, uint64_t target) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < target) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------
// projection of one point: render.cu:33-40 (matmul rows 0..2), :63 (z cull),
// :65-66 (rintf of the quotient), :68 (frustum cull), :70 (pixel id).
// Returns pixel id or -1.
__device__ __forceinline__ int project_point(const Proj &P, float x, float y, float z, int W, int H, float fW,
                                             float fH, float &depth) {
    float rx = f_add(fmaf(P.m[2], z, fmaf(P.m[1], y, f_mul(P.m[0], x))), P.m[3]);
    float ry = f_add(fmaf(P.m[6], z, fmaf(P.m[5], y, f_mul(P.m[4], x))), P.m[7]);
    float rz = f_add(fmaf(P.m[10], z, fmaf(P.m[9], y, f_mul(P.m[8], x))), P.m[11]);
    float inv = 1.0f / rz;  // correctly rounded (v_div_scale / v_div_fmas / v_div_fixup)
    float fu = rintf(f_mul(rx, inv));
    float fv = rintf(f_mul(ry, inv));
    bool ok = (rz > 0.0f) && (fu >= 0.0f) && (fu < fW) && (fv >= 0.0f) && (fv < fH);
    depth = rz;
    return ok ? ((int)fv * W + (int)fu) : -1;
}

typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_stream(const float4 *p) {
    v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// inclusive scan over the workgroup (<= 8 waves); returns the inclusive prefix, `total` = sum of all
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *s_w /*[8]*/, uint32_t &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    __syncthreads();  // s_w may still be read from the previous scan
    if (lane == 63) s_w[wv] = v;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    for (int k = 0; k < nw; ++k) {
        const uint32_t w = s_w[k];
        base += k < wv ? w : 0u;
        total += w;
    }
    return v + base;
}

// PackedXyz helpers ---------------------------------------------------------------
// An axis block is TWO little-endian bit streams (rtr_kernels.h): the FIRST value of every lane -- lane l's b bits at bit
// b l of the A stream, 8 b bytes -- and its other three -- 3 b bits at bit 3 b l of the B stream, 24 b bytes.  A lane
// reads the 8 (16) bytes that start at the DWORD holding its first bit (loads whose lane stride is not a multiple of
// four bytes run at a third of the rate: 2.2-3.8 TB/s against 7.0, tools/align_probe.hip) and shifts its data down by
// the remaining 0..31 bits; b <= 25 keeps shift + b <= 64 and shift + 3 b <= 128.  A fixed number of loads per chunk,
// no branch around any of them; both streams end with spare bytes for the last lane's over-read.
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
struct AxisRawA { uint32_t d[2]; };
struct AxisRaw { uint32_t d[4]; };
__device__ __forceinline__ AxisRawA ld_axis_a(const uint8_t *block, uint32_t b, int lane) {
    const uint32_t dw = (b * (uint32_t)lane) >> 5;
    const u32x2_a4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_a4 *>(block + 4u * dw));
    return AxisRawA{{v.x, v.y}};
}
__device__ __forceinline__ AxisRaw ld_axis_b(const uint8_t *block, uint32_t b, int lane) {
    const uint32_t dw = (3u * b * (uint32_t)lane) >> 5;
    const u32x4_a4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a4 *>(block + 4u * dw));
    return AxisRaw{{v.x, v.y, v.z, v.w}};
}
// value 0 = base | the lane's b bits of the A stream, value k = base | bits [b (k - 1), b k) of its realigned B data.
// Branch-free for every b <= 25 (b = 0: the mask is empty and the value is the base).  A first version picked the dwords
// a value straddles by width class behind wave-uniform branches: ~10 branches per axis made the point kernel 14 us
// slower than the byte-granular form it was meant to beat.  b is wave-uniform.
__device__ __forceinline__ float4 unpack_axis_narrow(const AxisRawA &ra, const AxisRaw &r, uint32_t b, uint32_t base, int lane) {
    // (a VOP3 instruction reads at most one scalar register on gfx950: with mask AND base scalar the compiler splits every
    // v_and_or into two instructions; the base in a vector register keeps it one)
    uint32_t vbase = base;
    asm("" : "+v"(vbase));
    uint32_t sha, shb;  // (b l) & 31, (3 b l) & 31: alignbit takes the low five bits of its shift
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(sha) : "s"(b), "v"(lane));
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(shb) : "s"(3u * b), "v"(lane));
    const uint32_t mask = (1u << b) - 1u;  // (b <= 25)
    const uint32_t a0 = __builtin_amdgcn_alignbit(ra.d[1], ra.d[0], sha);
    const uint32_t e0 = __builtin_amdgcn_alignbit(r.d[1], r.d[0], shb), e1 = __builtin_amdgcn_alignbit(r.d[2], r.d[1], shb);
    const uint32_t e2 = __builtin_amdgcn_alignbit(r.d[3], r.d[2], shb);
    const uint32_t f0 = __builtin_amdgcn_alignbit(e1, e0, b), f1 = __builtin_amdgcn_alignbit(e2, e1, b);
    const uint32_t g0 = __builtin_amdgcn_alignbit(f1, f0, b);
    auto and_or = [&](uint32_t e) -> float {  // (the compiler leaves v_and + v_or here)
        uint32_t x;
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(x) : "v"(e), "s"(mask), "v"(vbase));
        return __uint_as_float(x);
    };
    return make_float4(and_or(a0), and_or(e0), and_or(f0), and_or(g0));
}
__device__ __forceinline__ float4 unpack_axis(const AxisRawA &ra, const AxisRaw &r, uint32_t b, uint32_t base, int lane) {
    if (b == 32u)  // (lane l's first value is dword l of the A stream, its other three dwords 3 l .. 3 l + 2 of the B stream)
        return make_float4(__uint_as_float(ra.d[0]), __uint_as_float(r.d[0]), __uint_as_float(r.d[1]), __uint_as_float(r.d[2]));
    return unpack_axis_narrow(ra, r, b, base, lane);
}
struct ChunkRawA { AxisRawA a[3]; };
struct ChunkRaw { AxisRaw a[3]; };
__device__ __forceinline__ ChunkRawA load_chunk_a(const uint32_t *__restrict__ planes_a, const uint4 &h0, const uint4 &h1, int lane) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(planes_a) + (((((uint64_t)h1.y) << 32) | (uint64_t)h1.x) << 3);
    ChunkRawA c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint32_t b = (h0.w >> (6 * a)) & 63u;
        c.a[a] = ld_axis_a(p, b, lane);
        p += 8u * b;
    }
    return c;
}
__device__ __forceinline__ ChunkRaw load_chunk_b(const uint32_t *__restrict__ planes_b, const uint4 &h0, const uint4 &h1, int lane) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(planes_b) + (((((uint64_t)h1.y) << 32) | (uint64_t)h1.x) * 24u);
    ChunkRaw c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint32_t b = (h0.w >> (6 * a)) & 63u;
        c.a[a] = ld_axis_b(p, b, lane);
        p += 24u * b;
    }
    return c;
}
__device__ __forceinline__ void unpack_chunk(const ChunkRawA &ca, const ChunkRaw &c, uint32_t widths, uint32_t bx, uint32_t by, uint32_t bz,
                                             float4 &X, float4 &Y, float4 &Z, int lane) {
    if (!(widths & kPackWideFlag)) {  // no axis of the chunk needs all 32 bits (the usual case)
        // (a constant axis -- a wall of the synthetic room, 30 % of its axis blocks -- skips the fifteen instructions)
        const uint32_t wx = widths & 63u, wy = (widths >> 6) & 63u, wz = (widths >> 12) & 63u;
        X = wx ? unpack_axis_narrow(ca.a[0], c.a[0], wx, bx, lane) : make_float4(__uint_as_float(bx), __uint_as_float(bx), __uint_as_float(bx), __uint_as_float(bx));
        Y = wy ? unpack_axis_narrow(ca.a[1], c.a[1], wy, by, lane) : make_float4(__uint_as_float(by), __uint_as_float(by), __uint_as_float(by), __uint_as_float(by));
        Z = wz ? unpack_axis_narrow(ca.a[2], c.a[2], wz, bz, lane) : make_float4(__uint_as_float(bz), __uint_as_float(bz), __uint_as_float(bz), __uint_as_float(bz));
    } else {
        X = unpack_axis(ca.a[0], c.a[0], widths & 63u, bx, lane);
        Y = unpack_axis(ca.a[1], c.a[1], (widths >> 6) & 63u, by, lane);
        Z = unpack_axis(ca.a[2], c.a[2], (widths >> 12) & 63u, bz, lane);
    }
}

__device__ __forceinline__ uint32_t spread_nibbles(uint32_t b) {  // bit m of the low byte -> bit 4 m
    uint32_t x = b & 0xFFu;
    x = (x | (x << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return x;
}

// The bits of upload-order words `keep` for the lane's four points of chunk c (rtr_remove_points, rtr_extract_points,
// rtr_transform_points): keep = the caller's words (bits at or past n ignored), perm = resident index -> upload index
// (null while the cloud is in upload order); u[k] = the upload index of point 4 lane + k, valid[k] = it lies below n,
// kept[k] = valid and its bit is set.
__device__ __forceinline__ void remove_gather(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ perm, uint64_t n,
                                              uint64_t c, int lane, uint32_t u[4], bool kept[4], bool valid[4]) {
    const uint64_t r0 = c * 256u + 4u * (uint64_t)lane;
    if (perm && r0 < n) {  // (perm holds whole quads: its arrays are padded to a multiple of 4 points)
        const uint4 q = *reinterpret_cast<const uint4 *>(perm + r0);
        u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = (uint32_t)(r0 + k);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        valid[k] = r0 + k < n;
        kept[k] = valid[k] && ((keep[u[k] >> 5] >> (u[k] & 31u)) & 1u);
    }
}

}  // namespace rtr
