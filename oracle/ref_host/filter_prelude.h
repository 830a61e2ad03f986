/* Force-included (after cuda_shim.h) in front of the kernel region cut from the reference's project_cloud.cu: the five
 * filter kernels need nothing but c10::Half, which the installed torch ships as a header-only type (its float <-> half
 * conversions are round-to-nearest-even bit manipulation on the host).  The project's own text. */
#pragma once
#include <c10/util/Half.h>
