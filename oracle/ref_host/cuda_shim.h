/* cuda_shim.h -- what the reference's KERNELS need from CUDA, for a host compiler (test infrastructure).
 *
 * Force-included (`g++ -x c++ -include cuda_shim.h`) in front of the reference's unchanged kernel text so that it
 * compiles as plain C++: one call of a kernel function is one CUDA thread, and ref_driver.cpp sets the four index
 * variables below before every call.  All of this file is the project's own text; nothing here is taken from the
 * reference.
 *
 *   qualifiers   __global__ / __device__ empty, __forceinline__ = inline, __shared__ empty (an `extern __shared__`
 *                array becomes an ordinary extern array that the driver defines), __constant__ = static const
 *   types        float4, uchar4, uint2, dim3
 *   indices      blockIdx, blockDim, threadIdx, gridDim: thread-local, written by the driver
 *   warp         a warp with ONE active lane: __activemask() is the calling lane's bit, __match_any_sync() returns
 *                the mask it is given, the reductions return their argument -- a legal execution of the kernels'
 *                text (the lane is always its own group's leader), and with the plain atomics below it gives the
 *                same memory image as any other, because min and integer addition are associative and commutative
 *   __fdividef   REF_FDIVIDEF_IEEE undefined: x * RN(1 / z), the project's contract;  defined: IEEE x / z.
 *                The hardware's approximate reciprocal is one of the two things a host build cannot decide.
 *   __syncthreads  empty: the driver launches the two kernels that use it with blockDim.x = 1 (see ref_driver.cpp)
 */
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__
#define __constant__ static const

struct float4 { float x, y, z, w; };
struct uchar4 { unsigned char x, y, z, w; };
struct uint2 { unsigned int x, y; };
struct dim3 { unsigned int x, y, z; };

/* __thread, not thread_local: a plain TLS access without the C++ initialisation wrapper */
extern __thread dim3 blockIdx, blockDim, threadIdx, gridDim;

using std::max;
using std::min;

template <class T> inline T __ldg(const T *p) { return *p; }

inline float __fdividef(float a, float b) {
#ifdef REF_FDIVIDEF_IEEE
    return a / b;
#else
    const float inv = 1.0f / b;
    return a * inv;
#endif
}

inline unsigned int __float_as_uint(float f) { unsigned int u; std::memcpy(&u, &f, sizeof u); return u; }
inline float __uint_as_float(unsigned int u) { float f; std::memcpy(&f, &u, sizeof f); return f; }

inline unsigned int __activemask() { return 1u << (threadIdx.x & 31u); }
inline unsigned int __match_any_sync(unsigned int mask, unsigned int) { return mask; }
inline unsigned int __reduce_min_sync(unsigned int, unsigned int v) { return v; }
inline unsigned int __reduce_add_sync(unsigned int, unsigned int v) { return v; }
inline int __ffs(unsigned int v) { return __builtin_ffs(static_cast<int>(v)); }
inline void __syncthreads() {}

inline uint32_t atomicMin(uint32_t *p, uint32_t v) { const uint32_t old = *p; if (v < old) *p = v; return old; }
inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p = old + v; return old; }
