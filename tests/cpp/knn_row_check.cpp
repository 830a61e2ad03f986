// rtr_knn_row.h -- the lines the rows kernel of rtr_select_statistical runs per lane -- on a plain array, against a sort.
// Built with g++ as a stand-alone program (and again with -fsanitize=address,undefined):
//   knn_row_check [trials]
// For every order of arrival below and k in {1, 2, 7, 8, 63, 64} the row after all insertions, sorted by knn_row_sort,
// must equal the min(k, n) smallest values of a std::sort by bits, the state must name the row's largest value and a
// slot that holds it, and knn_row_mean must be the sequential fp32 sum of square roots divided by the count.  The row
// lives in a heap block of exactly k floats, so an access past the row is the sanitizer's to report.
// Orders: random values (many ties: drawn from few distinct ones; and all distinct), ascending, descending, all equal,
// ties at the worst value (a full row of w followed by more w, then one smaller), fewer than k values, none, and
// subnormal and zero values.  Exit 1 with a message on the first difference.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "rtr_knn_row.h"

struct HeapRow {
    std::unique_ptr<float[]> v;
    uint32_t k;
    unsigned long reads = 0, writes = 0;
    explicit HeapRow(uint32_t k_) : v(new float[k_]), k(k_) {}
    float get(uint32_t s) const { if (s >= k) { fprintf(stderr, "get(%u) past the row of %u\n", s, k); exit(1); } return v[s]; }
    void set(uint32_t s, float x) { if (s >= k) { fprintf(stderr, "set(%u) past the row of %u\n", s, k); exit(1); } v[s] = x; ++writes; }
};

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int check(const char* what, uint32_t k, const std::vector<float>& in) {
    HeapRow row(k);
    rtr::KnnRowState st;
    unsigned long written = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        const rtr::KnnRowState before = st;
        const bool took = rtr::knn_row_insert(row, k, st, in[i]);
        written += took;
        // a full row takes a value iff it is smaller than the worst; a row that is not full takes everything
        const bool must = before.count < k || in[i] < before.worst;
        if (took != must) { fprintf(stderr, "%s k=%u: value %zu taken=%d, expected %d\n", what, k, i, (int)took, (int)must); return 1; }
        if (st.count != std::min<size_t>(k, i + 1)) { fprintf(stderr, "%s k=%u: count %u after %zu values\n", what, k, st.count, i + 1); return 1; }
        float w = row.get(0);
        for (uint32_t s = 1; s < st.count; ++s) w = std::max(w, row.get(s));
        if (bits(w) != bits(st.worst) || st.worst_slot >= st.count || bits(row.get(st.worst_slot)) != bits(w)) {
            fprintf(stderr, "%s k=%u: after value %zu the state names %g in slot %u, the row's worst is %g\n", what, k, i, st.worst, st.worst_slot, w);
            return 1;
        }
    }
    if (written != row.writes) { fprintf(stderr, "%s k=%u: %lu values taken but %lu stores\n", what, k, written, row.writes); return 1; }
    rtr::knn_row_sort(row, st.count);
    std::vector<float> want(in);
    std::sort(want.begin(), want.end(), [](float a, float b) { return bits(a) < bits(b); });
    want.resize(std::min<size_t>(k, want.size()));
    if (st.count != want.size()) { fprintf(stderr, "%s k=%u: %u values kept, expected %zu\n", what, k, st.count, want.size()); return 1; }
    for (uint32_t s = 0; s < st.count; ++s)
        if (bits(row.get(s)) != bits(want[s])) { fprintf(stderr, "%s k=%u: slot %u holds %a, expected %a\n", what, k, s, row.get(s), want[s]); return 1; }
    volatile float sum = 0.f;  // (volatile: every sum rounded to fp32 on its own, whatever the compiler's excess precision)
    for (float d2 : want) { volatile float r = sqrtf(d2); sum = sum + r; }
    const float mean = want.empty() ? INFINITY : sum / (float)want.size();
    const float got = rtr::knn_row_mean(row, st.count);
    if (bits(got) != bits(mean)) { fprintf(stderr, "%s k=%u: mean %a, expected %a\n", what, k, got, mean); return 1; }
    return 0;
}

int main(int argc, char** argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 200;
    std::mt19937 rng(12345);
    const uint32_t ks[] = {1, 2, 7, 8, 63, 64};
    unsigned long cases = 0;
    for (uint32_t k : ks) {
        for (int t = 0; t < trials; ++t) {
            const size_t n = rng() % (4 * k + 3);
            std::vector<float> a(n);
            const int distinct = 1 + (int)(rng() % 6);
            for (float& x : a) x = (t & 1) ? (float)(rng() % distinct) * 0.125f : (float)(rng() >> 8) * (1.0f / 16777216.0f);
            if (check("random", k, a)) return 1;
            std::vector<float> up(a), down(a);
            std::sort(up.begin(), up.end());
            std::sort(down.begin(), down.end(), std::greater<float>());
            if (check("ascending", k, up) || check("descending", k, down)) return 1;
            cases += 3;
        }
        for (size_t n : {(size_t)0, (size_t)1, (size_t)k - 1, (size_t)k, (size_t)k + 1, (size_t)3 * k}) {
            if (check("all equal", k, std::vector<float>(n, 0.25f))) return 1;
            if (check("all zero", k, std::vector<float>(n, 0.0f))) return 1;
            std::vector<float> ties(n, 0.5f);  // ties at the worst value, then one that beats them, then ties again
            ties.push_back(0.125f);
            ties.insert(ties.end(), n, 0.5f);
            ties.push_back(0.125f);
            if (check("ties at the worst", k, ties)) return 1;
            std::vector<float> tiny;
            for (size_t i = 0; i < n; ++i) tiny.push_back(i % 3 == 0 ? 0.0f : ldexpf((float)(1 + (rng() % 1000)), -149));
            if (check("subnormal", k, tiny)) return 1;
            cases += 4;
        }
    }
    printf("%lu cases, %d trials per k\n", cases, trials);
    return 0;
}
