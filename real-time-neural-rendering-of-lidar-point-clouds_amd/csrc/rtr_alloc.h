// rtr_alloc.h -- the library's one allocation path: every device and pinned-host allocation and every free of csrc/
// goes through the functions below (tests/test_alloc_failure_host.py refuses a bare hipMalloc / hipFree anywhere else),
// so that the failure switch of rtr_alloc_rule.h reaches every allocation site and the live count sees every buffer.
//
// When the switch fires the call returns hipErrorOutOfMemory without calling HIP and stores NULL: it never hands back a
// pointer that is not a live allocation.  A real failure stores NULL too, whatever the runtime left in *p.
#pragma once
#include <hip/hip_runtime.h>

#include "rtr_alloc_rule.h"

namespace rtr {

inline hipError_t dev_malloc_flags(void **p, size_t bytes, bool uncached) {
    *p = nullptr;
    if (alloc_rule().attempt_fails()) return hipErrorOutOfMemory;
    const hipError_t e = uncached ? hipExtMallocWithFlags(p, bytes, hipDeviceMallocUncached) : hipMalloc(p, bytes);
    if (e == hipSuccess) alloc_rule().made(); else *p = nullptr;
    return e;
}
template <class T> hipError_t dev_malloc(T **p, size_t bytes) { return dev_malloc_flags((void **)p, bytes, false); }
template <class T> hipError_t dev_malloc_uncached(T **p, size_t bytes) { return dev_malloc_flags((void **)p, bytes, true); }

template <class T> hipError_t host_malloc(T **p, size_t bytes, unsigned flags) {  // pinned host memory
    *p = nullptr;
    if (alloc_rule().attempt_fails()) return hipErrorOutOfMemory;
    void *q = nullptr;
    const hipError_t e = hipHostMalloc(&q, bytes, flags);
    if (e == hipSuccess) alloc_rule().made(); else q = nullptr;
    *p = static_cast<T *>(q);
    return e;
}

// (NULL is nobody's allocation: nothing is freed or counted)
inline hipError_t dev_free(void *p) {
    if (!p) return hipSuccess;
    alloc_rule().freed();
    return hipFree(p);
}
inline hipError_t host_free(void *p) {
    if (!p) return hipSuccess;
    alloc_rule().freed();
    return hipHostFree(p);
}

}  // namespace rtr
