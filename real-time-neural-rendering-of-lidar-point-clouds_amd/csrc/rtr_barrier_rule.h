// rtr_barrier_rule.h -- the wait condition of the peer-to-peer flag barrier (k_p2p_sync, k_p2p_sync_gather in
// rtr_kernels.hip): one function that both kernels call, and that tests/cpp/barrier_rule_check.cpp compiles with g++.
//
// A rank entering barrier number `seq` stores seq into its flag word on every peer and waits until each peer's word
// on this rank has reached seq.  The counter is 32 bits wide and wraps after 2^32 barriers, so "has reached" is a
// serial-number comparison (RFC 1982): the difference flag - seq, taken modulo 2^32 and read as a signed number, is
// negative exactly while the peer is behind.  All ranks run the same sequence of barriers and a rank never runs
// ahead of a peer by more than one, so the two values are always far closer than the 2^31 the comparison can tell
// apart.  A plain `flag < seq` fails in a window around the wrap: a rank whose seq has wrapped to a small value does not
// wait for a peer whose word still holds a number from before the wrap (barrier 0 waits for nobody at all), so it may
// run any number of barriers ahead of a peer that has not passed 0 yet, and flags no timeout; once every rank has
// passed 0 the plain comparison orders them again.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTR_BARRIER_FN __host__ __device__ inline
#else
#define RTR_BARRIER_FN inline
#endif

namespace rtr {

// the peer whose flag word reads `flag` has not yet arrived at barrier `seq`
RTR_BARRIER_FN bool barrier_not_arrived(uint32_t flag, uint32_t seq) { return (int32_t)(flag - seq) < 0; }

}  // namespace rtr
