// rtr_union_find.h -- the lock-free union-find over sorted positions that rtr_clusters.hip (rtr.h section 6i) and
// rtr_segments.hip (rtr_segments.h section 6q) link their accepted pairs with.  Device-only, like rtr_device.h: every
// function is __device__ __forceinline__, so no device call crosses a translation unit.  Included by those two files
// and nothing else.
#pragma once
#include "rtr_device.h"

namespace rtr {

// ---------------------------------------------------------------------------------
// Union-find over sorted positions.
// INVARIANT, at every instant and for every v: parent[v] <= v.  It holds by construction: k_cl_init writes the identity;
// the only stores behind it are (a) the hook, atomicCAS(parent + hi, hi, lo) with lo < hi, and (b) the shortcut,
// atomicMin(parent + v, g) -- which can only lower a word.  So parent[v] never rises, a word that once differed from
// its index differs for good (a position that stopped being a root never becomes one again; only roots are hooked,
// since the CAS expects parent[hi] == hi), and every walk v -> parent[v] -> ... strictly decreases until it meets a word
// equal to its index: it ends after at most v steps whatever other waves do and however old the values it reads are.
// No wave ever waits for another one: there is no lock and no spin on a value someone else has to write.
// Every read of parent[] in k_cl_link is a relaxed agent-scope atomic load (an sc1 load served by L2): a plain load
// may be served by the CU's L1 with a value that another CU has replaced within this launch.  An old value is still
// safe -- it is an earlier ancestor of the same set, and >= the current one -- only slower.
__device__ __forceinline__ uint32_t ld_parent(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v's set as seen now; on the way every visited position is pointed at its grandparent (path splitting),
// by atomicMin: g is an ancestor of v, so g < v, and the word only falls
__device__ __forceinline__ uint32_t cl_find(uint32_t *parent, uint32_t v) {
    uint32_t p = ld_parent(parent + v);
    while (p != v) {  // (p < v: strictly decreasing)
        const uint32_t g = ld_parent(parent + p);
        if (g != p) atomicMin(parent + v, g);
        v = p, p = g;
    }
    return v;
}

// Unites the sets of a and b; returns a position of the united set that is <= both roots found (the next walk's start).
// The larger root is hooked under the smaller one.  A CAS that fails returns the word another wave has put there,
// which is < hi: the next round starts from it, so max(a, b) falls strictly with every failed round and the loop ends
// after finitely many rounds even if every load were arbitrarily old.
__device__ __forceinline__ uint32_t cl_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cl_find(parent, a), b = cl_find(parent, b);
        if (a == b) return a;  // (one set already: no store)
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        a = old, b = lo;  // (old < hi: hi has been hooked elsewhere meanwhile)
    }
}

}  // namespace rtr
