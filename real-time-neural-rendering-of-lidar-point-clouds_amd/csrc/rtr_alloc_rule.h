// rtr_alloc_rule.h -- the decision "does this allocation attempt fail" and the allocation counters, free of HIP: the
// wrappers of rtr_alloc.h ask it before every hipMalloc / hipHostMalloc, and tests/cpp/alloc_rule_check.cpp compiles it
// with g++.
//
// A test aid (options "debug_alloc_fail", "debug_alloc_count", "debug_alloc_live", rtr.h): armed at N >= 1, the N-th
// attempt from then on is told to fail, once, and the switch disarms itself; every other attempt goes through.  The
// wrapper then returns hipErrorOutOfMemory WITHOUT calling HIP, so nothing absurd is ever requested from the device,
// nothing is launched and HIP's sticky last error stays clean.  The state is process-wide: rtr_reorder.hip and DevBufs
// allocate with no context at hand, and a test reads the live count through a context of its own.
//
// Cost when the switch is off, i.e. always outside the tests: one relaxed load of `countdown` and two relaxed
// increments per allocation; a steady-state frame allocates nothing.
#pragma once
#include <stdint.h>

#include <atomic>

namespace rtr {

struct AllocRule {
    std::atomic<int64_t> countdown{0};  // attempts still to go until one fails (that one included); 0: off
    std::atomic<uint64_t> attempts{0};  // allocation attempts so far, failed ones included
    std::atomic<int64_t> live{0};       // allocations made and not yet freed

    // the N-th attempt from now on fails (N >= 1); N <= 0 disarms
    void arm(int64_t n) { countdown.store(n > 0 ? n : 0, std::memory_order_relaxed); }
    // attempts still to go; 0 once it has fired or is off
    int64_t remaining() const { return countdown.load(std::memory_order_relaxed); }

    // One allocation attempt: counted, and true when it is the one that has to fail.  With several threads attempting
    // at once the compare-exchange hands the step 1 -> 0 to exactly one of them.
    bool attempt_fails() {
        attempts.fetch_add(1, std::memory_order_relaxed);
        int64_t v = countdown.load(std::memory_order_relaxed);
        while (v > 0)
            if (countdown.compare_exchange_weak(v, v - 1, std::memory_order_relaxed)) return v == 1;
        return false;
    }
    void made() { live.fetch_add(1, std::memory_order_relaxed); }
    void freed() { live.fetch_sub(1, std::memory_order_relaxed); }
};

inline AllocRule &alloc_rule() {  // the process's one instance
    static AllocRule r;
    return r;
}

}  // namespace rtr
