// rtr_overlap_policy.h -- when whole-frame renders run overlapped (option "overlap", rtr.h): the streak / engage / leave
// decisions of rtr_render, host only and free of HIP (tests/cpp/overlap_policy_check.cpp compiles it with g++).
//
// Option "overlap": 0 never, 1 every whole frame that can (the caller paid for the second tile store when it set the
// option), -1 automatic: from the kEngageAt-th consecutive rtr_render of a context on -- the same resolution and cloud,
// the tile form, one GPU, no peer-to-peer exchange open, frames with the prefilter -- and only while the second store
// and pool could be had.  Every other entry point of the library ends the streak (other_call); the next one starts at
// frame 1.
// Frames without the prefilter are left alone by the automatic mode because they lose: their tail is the tile kernel
// alone, the kernel that stretches most beside T1, and the hand-over between the two streams is then not hidden by
// anything (measured from 1e7 to 7e7 points: +1 to +9 % per frame, against -13 to -18 % with the prefilter).
#pragma once
#include <stdint.h>

namespace rtr {

struct OverlapPolicy {
    static constexpr int kEngageAt = 3;

    int mode = 0;               // option "overlap": -1, 0, 1
    int streak = 0;             // consecutive eligible whole frames so far (saturates at kEngageAt)
    bool active = false;        // the last whole frame ran overlapped
    bool alloc_failed = false;  // automatic only: the second set could not be allocated -- serial until something changes
    int W = 0, H = 0;           // what the streak was counted for
    uint64_t cloud = 0;

    void set_mode(int m) {
        mode = m < 0 ? -1 : (m > 0 ? 1 : 0);
        streak = 0;
        active = false;
        alloc_failed = false;
    }

    // Anything but rtr_render was called: the streak is over
    void other_call() {
        streak = 0;
        active = false;
    }

    // A whole frame is about to be queued.  eligible: the tile form, one GPU, no exchange open; pays: it has the
    // prefilter (asked of the automatic mode only).  Returns whether the frame should run overlapped -- the caller then
    // makes sure of the second set and reports a failure with resources_failed(), and every frame ends with frame_done()
    bool frame(bool eligible, bool pays, int w, int h, uint64_t cloud_seq) {
        if (w != W || h != H || cloud_seq != cloud) {  // (another resolution or cloud: count again, and try the allocation again)
            W = w, H = h, cloud = cloud_seq;
            streak = 0;
            alloc_failed = false;
        }
        if (!eligible || mode == 0 || (mode < 0 && !pays)) {
            streak = 0;
            return false;
        }
        if (streak < kEngageAt) ++streak;
        if (mode == 1) return true;
        return streak >= kEngageAt && !alloc_failed;
    }

    void resources_failed() { alloc_failed = true; }  // (the frame that asked runs serially, and so do the next)

    void frame_done(bool overlapped) { active = overlapped; }
};

}  // namespace rtr
