// rtr_topk_cascade.h on the CPU: the very lines rtr_nearest_k.hip runs, on std::atomic<uint64_t> from 2 .. 8 threads.
// Rows of k = 1 .. 64 slots, 0 .. 300 distinct keys per row, their high halves ("d2 bits") drawn from a handful of
// values so that most keys tie there and differ in the low half ("index") alone.  The keys of a trial are dealt to the
// threads, every thread inserts its share into the rows in its own order, all threads at once: plainly, with the prune (a
// relaxed read of row[k - 1] first, the key dropped when it does not beat it), and with the prune and the skip (the row
// read slot by slot first, the walk started behind the leading slots read below the key).  After the join every row must equal
// the sorted k smallest keys with all ones behind them.  Exit 0 when every trial agrees, 1 with a message otherwise.
//   topk_cascade_check [trials]
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "rtr_topk_cascade.h"

static uint64_t fetch_min(std::atomic<uint64_t>& a, uint64_t v) {  // (std::atomic has no fetch_min before C++26)
    uint64_t old = a.load(std::memory_order_relaxed);
    while (old > v && !a.compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
    return old;
}

struct Item { uint32_t row; uint64_t key; };

int main(int argc, char** argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 400;
    std::mt19937_64 rng(12345);
    for (int t = 0; t < trials; ++t) {
        const uint32_t k = t < 192 ? (uint32_t)t / 3u + 1u : 1u + (uint32_t)(rng() % 64);  // (every k in each of the three modes)
        const int threads = 2 + (int)(rng() % 7);
        const bool prune = t % 3 != 0, skip = t % 3 == 2;
        const uint32_t rows = 1u + (uint32_t)(rng() % 6);
        const uint32_t levels = 1u + (uint32_t)(rng() % 5);  // distinct "d2 bits" per trial: heavy ties
        std::vector<std::vector<uint64_t>> keys(rows);
        std::vector<std::vector<Item>> share(threads);
        for (uint32_t r = 0; r < rows; ++r) {
            const uint32_t count = (uint32_t)(rng() % 301);
            std::vector<uint32_t> index(count);
            for (uint32_t i = 0; i < count; ++i) index[i] = i * 7u + (uint32_t)(rng() % 7);  // (distinct)
            std::shuffle(index.begin(), index.end(), rng);
            for (uint32_t i = 0; i < count; ++i) {
                const uint64_t key = ((uint64_t)(0x3A000000u + (uint32_t)(rng() % levels)) << 32) | index[i];
                keys[r].push_back(key);
                share[rng() % threads].push_back({r, key});
            }
        }
        std::vector<std::atomic<uint64_t>> slots((size_t)rows * k);
        for (auto& s : slots) s.store(rtr::kTopkEmpty, std::memory_order_relaxed);
        std::atomic<int> go{0};
        std::vector<std::thread> pool;
        for (int w = 0; w < threads; ++w) {
            pool.emplace_back([&, w] {
                go.fetch_add(1);
                while (go.load() < threads) {}  // (start together)
                for (const Item& it : share[w]) {
                    std::atomic<uint64_t>* row = slots.data() + (size_t)it.row * k;
                    if (prune && !rtr::topk_beats(it.key, row[k - 1].load(std::memory_order_relaxed))) continue;
                    uint32_t first = 0;
                    if (skip) {
                        uint64_t snap[64];  // (read before anything is decided: stale by the time it is used)
                        for (uint32_t s = 0; s < k; ++s) snap[s] = row[s].load(std::memory_order_relaxed);
                        while (first < k && snap[first] < it.key) ++first;
                    }
                    rtr::topk_cascade(k, it.key, [row](uint32_t s, uint64_t v) { return fetch_min(row[s], v); }, first);
                }
            });
        }
        for (auto& th : pool) th.join();
        for (uint32_t r = 0; r < rows; ++r) {
            std::sort(keys[r].begin(), keys[r].end());
            for (uint32_t s = 0; s < k; ++s) {
                const uint64_t want = s < keys[r].size() ? keys[r][s] : rtr::kTopkEmpty;
                const uint64_t got = slots[(size_t)r * k + s].load();
                if (got != want) {
                    fprintf(stderr, "trial %d (k %u, %d threads, prune %d, skip %d): row %u slot %u holds %016llx, not %016llx\n", t, k, threads, (int)prune,
                            (int)skip, r, s, (unsigned long long)got, (unsigned long long)want);
                    return 1;
                }
            }
        }
    }
    printf("%d trials\n", trials);
    return 0;
}
