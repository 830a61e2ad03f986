// rtr_register.hip -- gfx950 kernels of rtr_register_points (include/rtr_register.h section 6p): one registration step of
// a scan against the resident cloud.  The correspondences are rtr_nearest_points' (rtr_nearest.hip's sweep, unchanged),
// the winners' coordinates come from one launch of rtr_kernels.hip's k_extract over scratch words; what is new here:
//   k_register_pose     the given points through the pose, in fp64, rounded to fp32: the records the search keys
//   k_register_mark     one bit per winner into scratch words (integer atomicOr; never the context's selection)
//   k_register_partial  the hot kernel: per given point its slot, its posed point, its winner's record and -- plane mode --
//                       its winner's normal; the terms of the pass in fp64; ALL sums of the pass folded in one launch,
//                       one set of partial sums per 1024 consecutive given indices, in section 6n's fixed shape
//   k_register_final    the partial sums into one set, in the same shape: one workgroup
// Templates on the mode and the pass: the 28 sums of the plane pass, the 10 of the point pass and the 7 of pass 0 each
// have their own register budget.  The arithmetic contract of rtr_kernels.hip holds (-ffp-contract=off: no FMA), fp32
// denormals are kept, and there is no floating-point atomic: every sum is a tree whose shape depends on count alone.
#include "rtr_device.h"
#include "rtr_register_kernels.h"

namespace rtr {

namespace {

constexpr int kRegChunk = 1024;
constexpr unsigned long long kNoSlot = ~0ull;

__global__ __launch_bounds__(kBlock) void k_register_pose(const uint8_t *__restrict__ xyz, uint64_t stride, uint64_t count, RegisterPose T,
                                                          float4 *__restrict__ out) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < count; j += (uint64_t)gridDim.x * kBlock) {
        const float *p = reinterpret_cast<const float *>(xyz + j * stride);
        float x = p[0], y = p[1], z = p[2];
        if (T.given) {
            const double X = (double)x, Y = (double)y, Z = (double)z;
            x = (float)(((T.t[0] * X + T.t[1] * Y) + T.t[2] * Z) + T.t[3]);
            y = (float)(((T.t[4] * X + T.t[5] * Y) + T.t[6] * Z) + T.t[7]);
            z = (float)(((T.t[8] * X + T.t[9] * Y) + T.t[10] * Z) + T.t[11]);
        }
        out[j] = make_float4(x, y, z, 1.0f);
    }
}

__global__ __launch_bounds__(kBlock) void k_register_mark(const unsigned long long *__restrict__ slots, uint64_t count, uint32_t *__restrict__ wsel) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < count; j += (uint64_t)gridDim.x * kBlock) {
        const unsigned long long key = slots[j];
        if (key == kNoSlot) continue;
        const uint32_t u = (uint32_t)key;
        atomicOr(wsel + (u >> 5), 1u << (u & 31u));
    }
}

template <bool PLANE, int PASS> struct RegSums { static constexpr int N = PASS == 0 ? 7 : (PLANE ? 28 : 10); };

__device__ __forceinline__ bool reg_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// v[] += the terms of given point j; a point without a used pair adds nothing (the bits of adding +0.0: no sum is ever -0)
template <bool PLANE, int PASS>
__device__ __forceinline__ void reg_add(const RegisterSums &a, uint64_t j, double (&v)[RegSums<PLANE, PASS>::N]) {
    const unsigned long long key = a.slots[j];
    if (key == kNoSlot) return;
    const uint32_t u = (uint32_t)key;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (PLANE) {
        const float f0 = a.normals[3ull * u], f1 = a.normals[3ull * u + 1], f2 = a.normals[3ull * u + 2];
        if (!(reg_finite(f0) && reg_finite(f1) && reg_finite(f2))) return;
        if (f0 == 0.f && f1 == 0.f && f2 == 0.f) return;
        n0 = (double)f0, n1 = (double)f1, n2 = (double)f2;
    }
    const uint32_t w = a.wsel[u >> 5];
    const float4 P = a.posed[j], Q = a.win[a.wscan[u >> 5] + (uint32_t)__popc(w & ((1u << (u & 31u)) - 1u))];
    const double p0 = (double)P.x, p1 = (double)P.y, p2 = (double)P.z, q0 = (double)Q.x, q1 = (double)Q.y, q2 = (double)Q.z;
    if (PASS == 0) {
        const double t[7] = {1.0, p0, p1, p2, q0, q1, q2};
#pragma unroll
        for (int k = 0; k < 7; ++k) v[k] = v[k] + t[k];
        return;
    }
    const double u0 = p0 - a.mean[0], u1 = p1 - a.mean[1], u2 = p2 - a.mean[2];
    if (!PLANE) {
        const double uu[3] = {u0, u1, u2}, vv[3] = {q0 - a.mean[3], q1 - a.mean[4], q2 - a.mean[5]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) v[3 * r + s] = v[3 * r + s] + uu[r] * vv[s];
        const double d0 = p0 - q0, d1 = p1 - q1, d2 = p2 - q2;
        v[9] = v[9] + ((d0 * d0 + d1 * d1) + d2 * d2);
    } else {
        const double aa[6] = {u1 * n2 - u2 * n1, u2 * n0 - u0 * n2, u0 * n1 - u1 * n0, n0, n1, n2};
        const double b = (n0 * (q0 - p0) + n1 * (q1 - p1)) + n2 * (q2 - p2);
        int at = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int s = r; s < 6; ++s, ++at) v[at] = v[at] + aa[r] * aa[s];
#pragma unroll
        for (int r = 0; r < 6; ++r) v[21 + r] = v[21 + r] + aa[r] * b;
        v[27] = v[27] + b * b;
    }
}

// The N values of every thread folded over the workgroup in section 6n's shape (rtr_statistical.hip's block_sum_fixed, N
// at a time): the 64 lanes by a butterfly, then the four waves in order; thread k < N returns sum k, the others +0.0
template <int N> __device__ __forceinline__ double reg_block_sums(double (&v)[N], double (*s_w)[4]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] = v[k] + __shfl_xor(v[k], off, 64);
    __syncthreads();  // (s_w may still be read from the previous round)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_w[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    const int k = threadIdx.x < (unsigned)N ? (int)threadIdx.x : 0;
    const double sum = ((s_w[k][0] + s_w[k][1]) + s_w[k][2]) + s_w[k][3];
    return threadIdx.x < (unsigned)N ? sum : 0.0;
}

template <bool PLANE, int PASS>
__global__ __launch_bounds__(kBlock) void k_register_partial(const RegisterSums a, double *__restrict__ partial) {
    constexpr int N = RegSums<PLANE, PASS>::N;
    __shared__ double s_w[N][4];
    const uint64_t nchunks = (a.count + kRegChunk - 1) / kRegChunk;
    for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {  // (workgroup-uniform)
        double v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = 0.0;
#pragma unroll
        for (int i = 0; i < kRegChunk / kBlock; ++i) {
            const uint64_t j = c * kRegChunk + (uint64_t)i * kBlock + threadIdx.x;
            if (j < a.count) reg_add<PLANE, PASS>(a, j, v);
        }
        const double sum = reg_block_sums<N>(v, s_w);
        if (threadIdx.x < (unsigned)N) partial[c * N + threadIdx.x] = sum;
    }
}

template <int N> __global__ __launch_bounds__(kBlock) void k_register_final(const double *__restrict__ partial, uint64_t nchunks, double *__restrict__ out) {
    __shared__ double s_w[N][4];
    double v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = 0.0;
    for (uint64_t c = threadIdx.x; c < nchunks; c += kBlock) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = v[k] + partial[c * N + k];
    }
    const double sum = reg_block_sums<N>(v, s_w);
    if (threadIdx.x < (unsigned)N) out[threadIdx.x] = sum;
}

unsigned flat_grid(uint64_t count) {
    const uint64_t blocks = (count + kBlock - 1) / kBlock;
    return (unsigned)(blocks < 4096 ? blocks : 4096);
}

template <bool PLANE, int PASS> void launch_sums(hipStream_t s, const RegisterSums &a, double *partial, double *out) {
    constexpr int N = RegSums<PLANE, PASS>::N;
    const uint64_t nchunks = register_chunks(a.count);
    if (nchunks) hipLaunchKernelGGL((k_register_partial<PLANE, PASS>), dim3((unsigned)(nchunks < 4096 ? nchunks : 4096)), dim3(kBlock), 0, s, a, partial);
    hipLaunchKernelGGL((k_register_final<N>), dim3(1), dim3(kBlock), 0, s, partial, nchunks, out);
}

}  // namespace

uint64_t register_chunks(uint64_t count) { return (count + kRegChunk - 1) / kRegChunk; }

void launch_register_pose(hipStream_t s, const uint8_t *xyz, uint64_t stride, uint64_t count, const RegisterPose &T, float4 *out) {
    if (count == 0) return;
    hipLaunchKernelGGL(k_register_pose, dim3(flat_grid(count)), dim3(kBlock), 0, s, xyz, stride, count, T, out);
}

void launch_register_mark(hipStream_t s, const uint64_t *slots, uint64_t count, uint32_t *wsel) {
    if (count == 0) return;
    hipLaunchKernelGGL(k_register_mark, dim3(flat_grid(count)), dim3(kBlock), 0, s, (const unsigned long long *)slots, count, wsel);
}

void launch_register_sums(hipStream_t s, const RegisterSums &a, bool plane, int pass, double *partial, double *out) {
    if (pass == 0) {
        if (plane) launch_sums<true, 0>(s, a, partial, out);
        else launch_sums<false, 0>(s, a, partial, out);
    } else if (plane) {
        launch_sums<true, 1>(s, a, partial, out);
    } else {
        launch_sums<false, 1>(s, a, partial, out);
    }
}

}  // namespace rtr
