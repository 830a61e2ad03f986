// Stub (the project's own text), see glm/detail/qualifier.hpp.  No arithmetic: the kernels build one ucvec4 and
// never compute with it, and the matrix composition (project_cloud.cu:318) is not compiled -- it stays unpinned.
#pragma once
#include "glm/detail/qualifier.hpp"
namespace glm {
template <int N, typename T, qualifier Q> struct vec {
    T data[N];
    vec() : data{} {}
    vec(T a, T b, T c) : data{a, b, c} { static_assert(N == 3, "three components"); }
    vec(T a, T b, T c, T d) : data{a, b, c, d} { static_assert(N == 4, "four components"); }
};
typedef vec<3, double, defaultp> dvec3;
}  // namespace glm
