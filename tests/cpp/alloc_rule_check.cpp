// The allocation failure switch and counters (csrc/rtr_alloc_rule.h) built with plain g++, alone: no HIP.
//
// Checked:
//   1. off by default: no attempt fails, every attempt is counted, remaining() reads 0;
//   2. armed at N, exactly the N-th attempt from then on fails and no other, before or behind it; remaining() counts
//      down N, N - 1, .. and reads 0 once it has fired: "fired" and "fewer than N attempts were made" differ;
//   3. the switch disarms itself: the attempts behind the failed one go through until it is armed again;
//   4. re-arming while armed starts over from the new N; arming at 0 or below disarms;
//   5. made() / freed() keep the live count;
//   6. with 2 .. 8 threads attempting at once, exactly one attempt fails, the count of attempts is exact, and the live
//      count returns to zero.  (tests/test_cpp_alloc_rule.py also runs this program built with -fsanitize=thread.)
// Prints "ok <checks>".
#include <cstdio>
#include <thread>
#include <vector>

#include "rtr_alloc_rule.h"

static long long checks = 0;
#define CHECK(cond)                                             \
    do {                                                        \
        ++checks;                                               \
        if (!(cond)) {                                          \
            printf("FAIL line %d: %s\n", __LINE__, #cond);      \
            return 1;                                           \
        }                                                       \
    } while (0)

int main() {
    rtr::AllocRule r;
    // 1. off by default
    CHECK(r.remaining() == 0);
    for (int i = 0; i < 1000; ++i) CHECK(!r.attempt_fails());
    CHECK(r.attempts.load() == 1000u && r.remaining() == 0 && r.live.load() == 0);

    // 2. + 3. armed at N: the N-th and no other; then off
    for (int n = 1; n <= 40; ++n) {
        const uint64_t before = r.attempts.load();
        r.arm(n);
        CHECK(r.remaining() == n);
        for (int i = 1; i <= n + 25; ++i) {
            CHECK(r.attempt_fails() == (i == n));
            CHECK(r.remaining() == (i < n ? n - i : 0));
        }
        CHECK(r.attempts.load() == before + (uint64_t)n + 25u);  // (the failed attempt is counted too)
    }
    // fewer than N attempts: it has not fired, and says so
    r.arm(5);
    for (int i = 0; i < 3; ++i) CHECK(!r.attempt_fails());
    CHECK(r.remaining() == 2);

    // 4. re-arming starts over; 0 and negative values disarm
    r.arm(2);
    CHECK(r.remaining() == 2);
    CHECK(!r.attempt_fails());
    r.arm(3);
    CHECK(!r.attempt_fails() && !r.attempt_fails() && r.attempt_fails() && !r.attempt_fails());
    r.arm(4);
    r.arm(0);
    CHECK(r.remaining() == 0);
    for (int i = 0; i < 10; ++i) CHECK(!r.attempt_fails());
    r.arm(-7);
    CHECK(r.remaining() == 0 && !r.attempt_fails());
    r.arm((int64_t)1 << 40);  // (wider than the option's int: the rule itself has no such limit)
    CHECK(r.remaining() == ((int64_t)1 << 40) && !r.attempt_fails() && r.remaining() == ((int64_t)1 << 40) - 1);
    r.arm(0);

    // 5. the live count
    r.made(); r.made(); r.made();
    CHECK(r.live.load() == 3);
    r.freed();
    CHECK(r.live.load() == 2);
    r.freed(); r.freed();
    CHECK(r.live.load() == 0);

    // the process's one instance is one instance
    CHECK(&rtr::alloc_rule() == &rtr::alloc_rule());
    CHECK(rtr::alloc_rule().remaining() == 0 && !rtr::alloc_rule().attempt_fails());

    // 6. threads: one failure, exact counts -- armed in the middle of what they will attempt together, at its first and
    // at its last attempt
    for (int threads = 2; threads <= 8; ++threads) {
        const int each = 2000;
        for (int64_t n : {(int64_t)1, (int64_t)threads * each / 2, (int64_t)threads * each}) {
            rtr::AllocRule t;
            t.arm(n);
            std::vector<int> failed((size_t)threads, 0);
            std::vector<std::thread> pool;
            for (int k = 0; k < threads; ++k)
                pool.emplace_back([&t, &failed, k, each]() {
                    for (int i = 0; i < each; ++i) {
                        if (t.attempt_fails()) {
                            ++failed[(size_t)k];
                        } else {
                            t.made();
                            t.freed();
                        }
                    }
                });
            for (auto &th : pool) th.join();
            int total = 0;
            for (int f : failed) total += f;
            CHECK(total == 1);
            CHECK(t.attempts.load() == (uint64_t)threads * each);
            CHECK(t.remaining() == 0 && t.live.load() == 0);
        }
        // armed beyond what they attempt: nobody fails, and the remainder is exact
        rtr::AllocRule t;
        t.arm((int64_t)threads * each + 9);
        std::vector<std::thread> pool;
        std::vector<int> failed((size_t)threads, 0);
        for (int k = 0; k < threads; ++k)
            pool.emplace_back([&t, &failed, k, each]() {
                for (int i = 0; i < each; ++i) failed[(size_t)k] += t.attempt_fails() ? 1 : 0;
            });
        for (auto &th : pool) th.join();
        int total = 0;
        for (int f : failed) total += f;
        CHECK(total == 0 && t.remaining() == 9);
    }
    printf("ok %lld\n", checks);
    return 0;
}
