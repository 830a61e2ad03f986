// Stub (the project's own text): glm is not a dependency of this repository.  The reference's types.h and render.cuh
// only name glm::vec<N, T, Q>, glm::defaultp and glm::dvec3; this is the least that lets them compile on the host.
#pragma once
namespace glm {
enum qualifier { defaultp };
template <int N, typename T, qualifier Q = defaultp> struct vec;
}  // namespace glm
