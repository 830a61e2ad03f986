// The streak / engage / leave decisions of option "overlap" (csrc/rtr_overlap_policy.h) built with plain g++: the
// automatic mode engages at the third consecutive whole frame and never earlier, every other call ends the streak and
// re-arms it, 0 and 1 override it, a failed allocation keeps the context serial, an open peer-to-peer exchange (an
// ineligible frame) makes it inactive, and so does a frame without the prefilter (which 1 overlaps all the same).
// Prints "ok <checks>".
#include <cstdio>

#include "rtr_overlap_policy.h"

static int checks = 0;
#define CHECK(cond)                                             \
    do {                                                        \
        ++checks;                                               \
        if (!(cond)) {                                          \
            printf("FAIL line %d: %s\n", __LINE__, #cond);      \
            return 1;                                           \
        }                                                       \
    } while (0)

// one whole frame as rtr_render drives the policy; alloc_ok: what the second set's allocation would answer
static bool frame(rtr::OverlapPolicy &p, bool eligible = true, bool alloc_ok = true, int w = 640, int h = 480,
                  uint64_t cloud = 1, bool filtered = true) {
    bool ov = p.frame(eligible, filtered, w, h, cloud);
    if (ov && !p.active && !alloc_ok) {
        p.resources_failed();
        ov = false;
    }
    p.frame_done(ov);
    return ov;
}

int main() {
    {   // automatic: the third frame, never earlier; stays on
        rtr::OverlapPolicy p;
        p.set_mode(-1);
        CHECK(!frame(p) && !p.active);
        CHECK(!frame(p) && !p.active);
        for (int k = 0; k < 50; ++k) CHECK(frame(p) && p.active);
    }
    {   // every kind of other call (the library funnels them all into other_call) at every point of a streak
        for (int at = 0; at < 6; ++at) {
            rtr::OverlapPolicy p;
            p.set_mode(-1);
            for (int k = 0; k < at; ++k) (void)frame(p);
            p.other_call();
            CHECK(!p.active);
            CHECK(!frame(p));
            CHECK(!frame(p));
            CHECK(frame(p));
            p.other_call();
            p.other_call();
            CHECK(!frame(p) && !frame(p) && frame(p) && frame(p));
        }
    }
    {   // a new resolution or cloud starts the count again
        rtr::OverlapPolicy p;
        p.set_mode(-1);
        CHECK(!frame(p) && !frame(p) && frame(p));
        CHECK(!frame(p, true, true, 96, 64));
        CHECK(!frame(p, true, true, 96, 64));
        CHECK(frame(p, true, true, 96, 64));
        CHECK(!frame(p, true, true, 96, 64, 2));
        CHECK(!frame(p, true, true, 96, 64, 2));
        CHECK(frame(p, true, true, 96, 64, 2));
    }
    {   // 0 and 1 override
        rtr::OverlapPolicy p;
        p.set_mode(0);
        for (int k = 0; k < 10; ++k) CHECK(!frame(p) && !p.active);
        p.set_mode(1);
        CHECK(!p.active);
        for (int k = 0; k < 10; ++k) CHECK(frame(p) && p.active);
        p.other_call();
        CHECK(!p.active && frame(p));  // (1: the first frame behind another call is overlapped again)
        p.set_mode(-1);
        CHECK(!p.active);
        CHECK(!frame(p) && !frame(p) && frame(p));
        p.set_mode(0);
        CHECK(!p.active && !frame(p));
        p.set_mode(7);
        CHECK(p.mode == 1);
        p.set_mode(-9);
        CHECK(p.mode == -1);
    }
    {   // the allocation fails: serial, no further attempt until the resolution, the cloud or the option changes
        rtr::OverlapPolicy p;
        p.set_mode(-1);
        CHECK(!frame(p) && !frame(p));
        CHECK(!frame(p, true, false) && !p.active && p.alloc_failed);
        for (int k = 0; k < 10; ++k) CHECK(!p.frame(true, true, 640, 480, 1));  // (does not even ask)
        p.other_call();
        for (int k = 0; k < 10; ++k) CHECK(!frame(p));
        CHECK(!frame(p, true, true, 320, 240) && !frame(p, true, true, 320, 240) && frame(p, true, true, 320, 240));
        CHECK(!frame(p, true, false) && !frame(p, true, false) && !frame(p, true, false) && p.alloc_failed);
        p.set_mode(-1);
        CHECK(!p.alloc_failed);
        CHECK(!frame(p) && !frame(p) && frame(p));
    }
    {   // an open exchange (ineligible frames): inactive, and the count starts when it closes
        rtr::OverlapPolicy p;
        p.set_mode(-1);
        for (int k = 0; k < 10; ++k) CHECK(!frame(p, false) && !p.active);
        CHECK(!frame(p) && !frame(p) && frame(p));
        CHECK(!frame(p, false) && !p.active);  // (opened inside a streak)
        CHECK(!frame(p) && !frame(p) && frame(p));
        p.set_mode(1);
        CHECK(!frame(p, false) && frame(p));
    }
    {   // frames without the prefilter: the automatic mode leaves them alone and counts again behind them
        rtr::OverlapPolicy p;
        p.set_mode(-1);
        for (int k = 0; k < 10; ++k) CHECK(!frame(p, true, true, 640, 480, 1, false) && !p.active);
        CHECK(!frame(p) && !frame(p) && frame(p) && frame(p));
        CHECK(!frame(p, true, true, 640, 480, 1, false) && !p.active);  // (inside a streak)
        CHECK(!frame(p) && !frame(p) && frame(p));
        p.set_mode(1);
        for (int k = 0; k < 4; ++k) CHECK(frame(p, true, true, 640, 480, 1, false) && p.active);
        p.set_mode(0);
        CHECK(!frame(p, true, true, 640, 480, 1, false) && !frame(p));
    }
    printf("ok %d\n", checks);
    return 0;
}
