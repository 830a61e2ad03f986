// rtr_register_kernels.h -- launch wrappers of rtr_register.hip (internal to librtr_hip.so): the kernels of
// rtr_register_points (include/rtr_register.h section 6p).  A header of its own beside rtr_kernels.h, which the frame
// path is compiled from and which stays as it is; the search is rtr_kernels.h's nearest_sweep, the winners' coordinates
// come from its launch_scan_u32 and launch_extract over scratch words.
#pragma once
#include "rtr_kernels.h"

namespace rtr {

// register_pose: out[j] = (the point at xyz + j * stride (DEVICE memory) through T in fp64, rounded to fp32; 1.0f); T.given
// == 0: the point as it is
struct RegisterPose { double t[12]; int given; };
void launch_register_pose(hipStream_t s, const uint8_t *xyz, uint64_t stride, uint64_t count, const RegisterPose &T, float4 *out);
// register_mark: wsel (upload-order words, zeroed by the caller) gets the bit of every slot's winner (integer atomicOr)
void launch_register_mark(hipStream_t s, const uint64_t *slots, uint64_t count, uint32_t *wsel);
// register_sums: out (device) = the sums of one pass over the `count` given points -- pass 0: the pairs used, sum p, sum q
// (7); pass 1: the nine sum u_a v_b and sum |p - q|^2 (10), or, plane, the 21 a_r a_s, the six a_r b and sum b^2 (28),
// about mean = (pbar, qbar) -- in fp64 and in a shape that depends on count alone.  slots: nearest_sweep's; posed:
// register_pose's; win: the winners' records in ascending upload index (launch_extract, stride 16) and wsel / wscan the
// words that name them and their exclusive popcount scan; normals (device, 3 n floats, upload order; plane only).
// partial: register_chunks(count) * 28 doubles of scratch
struct RegisterSums {
    const uint64_t *slots;
    const float4 *posed, *win;
    const uint32_t *wsel, *wscan;
    const float *normals;
    uint64_t count;
    double mean[6];
};
uint64_t register_chunks(uint64_t count);
void launch_register_sums(hipStream_t s, const RegisterSums &a, bool plane, int pass, double *partial, double *out);

}  // namespace rtr
