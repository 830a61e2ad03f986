// rtr_normal_fit.h -- the lines the rows kernel of rtr_estimate_normals runs per lane -- on plain arrays.  Built with g++
// as a stand-alone program (-ffp-contract=off -fno-fast-math; and again with -fsanitize=address,undefined):
//   normal_fit_check <trials> [<in.bin> <out.bin>]
// 1. The row.  For every order of arrival below and k in {1, 2, 7, 8, 63, 64} the row after all insertions, sorted by
//    normal_row_sort, must equal the min(k, n) smallest entries of a std::sort by (d2 bits, upload index); an entry must
//    be taken iff the row is not full or the entry is below the row's worst in that order; the state must name the
//    row's largest entry.  The row lives in heap blocks of exactly k entries, so an access past it is the sanitizer's to
//    report.  Orders: random values (many ties: drawn from few distinct ones; and all distinct), ascending, descending,
//    all equal (the index alone decides, arriving ascending, descending and shuffled), ties at the worst value, fewer
//    than k values, none, subnormal and zero values.  The position of an entry is NOT its index: index_of goes through
//    a shuffled table, as the kernel's goes through the sorted records.
// 2. The fit.  <in.bin>: u64 n, u32 k, u32 with_view, 3 floats the viewpoint, n * 3 floats the coordinates, n u32 found,
//    n * k u32 the rows' upload indices as tests/normals_ref.py dumps them.  For every point with found >= 2 the program
//    forms the float differences, the nine fp64 sums in row order and normal_fit; the others get (0, 0, 0) and +inf.
//    <out.bin>: n * 3 floats, n floats, n bytes (negated by the viewpoint rule).
// 3. sqrt_rn must return the builtin's value on this host for every argument seen in 1. and 2.: the fix-up is a no-op
//    where sqrt is correctly rounded.  The program prints "<cases> cases, <trials> trials per k, <roots> square roots".
// Exit 1 with a message on the first difference.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

static unsigned long g_roots = 0, g_fixed = 0;
static void root_seen(double x, double y0, double y) {
    ++g_roots;
    if (memcmp(&y0, &y, sizeof y) != 0 || !(y0 == std::sqrt(x) || x != x)) ++g_fixed;
}
#define RTR_SQRT_RN_HOOK(x, y0, y) root_seen(x, y0, y)
#include "rtr_normal_fit.h"

struct Entry { float d2; uint32_t u; };

struct HeapRow {
    std::unique_ptr<float[]> d;
    std::unique_ptr<uint32_t[]> p;
    uint32_t k;
    unsigned long writes = 0;
    explicit HeapRow(uint32_t k_) : d(new float[k_]), p(new uint32_t[k_]), k(k_) {}
    void in(uint32_t s) const { if (s >= k) { fprintf(stderr, "slot %u past the row of %u\n", s, k); exit(1); } }
    float d2(uint32_t s) const { in(s); return d[s]; }
    uint32_t pos(uint32_t s) const { in(s); return p[s]; }
    void set(uint32_t s, float x, uint32_t at) { in(s); d[s] = x, p[s] = at; ++writes; }
};

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool below(const Entry& a, const Entry& b) { return bits(a.d2) < bits(b.d2) || (bits(a.d2) == bits(b.d2) && a.u < b.u); }

// in[i] arrives i-th; its position is i and its upload index in[i].u (distinct)
static int check(const char* what, uint32_t k, const std::vector<Entry>& in) {
    HeapRow row(k);
    rtr::NormalRowState st;
    auto index_of = [&](uint32_t pos) { if (pos >= in.size()) { fprintf(stderr, "index_of(%u)\n", pos); exit(1); } return in[pos].u; };
    unsigned long written = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        const rtr::NormalRowState before = st;
        const bool must = before.count < k || below(in[i], Entry{row.d2(before.worst_slot), index_of(row.pos(before.worst_slot))});
        const bool took = rtr::normal_row_insert(row, k, st, index_of, in[i].d2, (uint32_t)i, in[i].u);
        written += took;
        if (took != must) { fprintf(stderr, "%s k=%u: entry %zu taken=%d, expected %d\n", what, k, i, (int)took, (int)must); return 1; }
        if (st.count != std::min<size_t>(k, i + 1)) { fprintf(stderr, "%s k=%u: count %u after %zu entries\n", what, k, st.count, i + 1); return 1; }
        uint32_t ws = 0;
        for (uint32_t s = 1; s < st.count; ++s)
            if (below(Entry{row.d2(ws), index_of(row.pos(ws))}, Entry{row.d2(s), index_of(row.pos(s))})) ws = s;
        if (st.worst_slot != ws || bits(st.worst) != bits(row.d2(ws))) {
            fprintf(stderr, "%s k=%u: after entry %zu the state names slot %u (%g), the row's worst is slot %u (%g)\n", what, k, i, st.worst_slot,
                    st.worst, ws, row.d2(ws));
            return 1;
        }
    }
    if (written != row.writes) { fprintf(stderr, "%s k=%u: %lu entries taken but %lu stores\n", what, k, written, row.writes); return 1; }
    rtr::normal_row_sort(row, st.count, index_of);
    std::vector<Entry> want(in);
    std::sort(want.begin(), want.end(), below);
    want.resize(std::min<size_t>(k, want.size()));
    if (st.count != want.size()) { fprintf(stderr, "%s k=%u: %u entries kept, expected %zu\n", what, k, st.count, want.size()); return 1; }
    for (uint32_t s = 0; s < st.count; ++s)
        if (bits(row.d2(s)) != bits(want[s].d2) || index_of(row.pos(s)) != want[s].u) {
            fprintf(stderr, "%s k=%u: slot %u holds (%a, %u), expected (%a, %u)\n", what, k, s, row.d2(s), index_of(row.pos(s)), want[s].d2, want[s].u);
            return 1;
        }
    return 0;
}

static std::vector<Entry> with_indices(const std::vector<float>& d2, int order, std::mt19937& rng) {
    std::vector<uint32_t> u(d2.size());
    for (size_t i = 0; i < u.size(); ++i) u[i] = 1000u + 3u * (uint32_t)i;
    if (order == 1) std::reverse(u.begin(), u.end());
    if (order == 2) std::shuffle(u.begin(), u.end(), rng);
    std::vector<Entry> e(d2.size());
    for (size_t i = 0; i < e.size(); ++i) e[i] = Entry{d2[i], u[i]};
    return e;
}

static int rows(int trials, unsigned long* cases) {
    std::mt19937 rng(12345);
    const uint32_t ks[] = {1, 2, 7, 8, 63, 64};
    for (uint32_t k : ks) {
        for (int t = 0; t < trials; ++t) {
            const size_t n = rng() % (4 * k + 3);
            std::vector<float> a(n);
            const int distinct = 1 + (int)(rng() % 6);
            for (float& x : a) x = (t & 1) ? (float)(rng() % distinct) * 0.125f : (float)(rng() >> 8) * (1.0f / 16777216.0f);
            std::vector<float> up(a), down(a);
            std::sort(up.begin(), up.end());
            std::sort(down.begin(), down.end(), std::greater<float>());
            for (int order = 0; order < 3; ++order) {
                if (check("random", k, with_indices(a, order, rng)) || check("ascending", k, with_indices(up, order, rng)) ||
                    check("descending", k, with_indices(down, order, rng)))
                    return 1;
                *cases += 3;
            }
        }
        for (size_t n : {(size_t)0, (size_t)1, (size_t)k - 1, (size_t)k, (size_t)k + 1, (size_t)3 * k}) {
            for (int order = 0; order < 3; ++order) {
                if (check("all equal", k, with_indices(std::vector<float>(n, 0.25f), order, rng))) return 1;
                if (check("all zero", k, with_indices(std::vector<float>(n, 0.0f), order, rng))) return 1;
                std::vector<float> ties(n, 0.5f);  // ties at the worst value, then one that beats them, then ties again
                ties.push_back(0.125f);
                ties.insert(ties.end(), n, 0.5f);
                ties.push_back(0.125f);
                if (check("ties at the worst", k, with_indices(ties, order, rng))) return 1;
                std::vector<float> tiny;
                for (size_t i = 0; i < n; ++i) tiny.push_back(i % 3 == 0 ? 0.0f : ldexpf((float)(1 + (rng() % 1000)), -149));
                if (check("subnormal", k, with_indices(tiny, order, rng))) return 1;
                *cases += 4;
            }
        }
    }
    return 0;
}

static int fit(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    unsigned long long n = 0;
    uint32_t k = 0, with_view = 0;
    float view[3];
    if (!f || fread(&n, 8, 1, f) != 1 || fread(&k, 4, 1, f) != 1 || fread(&with_view, 4, 1, f) != 1 || fread(view, 4, 3, f) != 3) return 2;
    std::vector<float> xyz(n * 3), normals(n * 3, 0.f), curv(n, INFINITY);
    std::vector<uint32_t> found(n), idx(n * k);
    std::vector<unsigned char> flipped(n, 0);
    if (fread(xyz.data(), 4, n * 3, f) != n * 3 || fread(found.data(), 4, n, f) != n || fread(idx.data(), 4, n * k, f) != n * k) return 2;
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        if (found[i] < 2u) continue;
        if (found[i] > k) { fprintf(stderr, "found[%zu] = %u > k\n", i, found[i]); return 1; }
        double S[3] = {0.0, 0.0, 0.0}, Q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const float* p = &xyz[i * 3];
        for (uint32_t t = 0; t < found[i]; ++t) {
            const uint32_t j = idx[i * k + t];
            if (j >= n) { fprintf(stderr, "row %zu slot %u names point %u\n", i, t, j); return 1; }
            const float* c = &xyz[(size_t)j * 3];
            volatile float dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];  // (volatile: rounded to fp32 whatever the excess precision)
            const double ex = (double)dx, ey = (double)dy, ez = (double)dz;
            S[0] = S[0] + ex, S[1] = S[1] + ey, S[2] = S[2] + ez;
            Q[0] = Q[0] + ex * ex, Q[1] = Q[1] + ex * ey, Q[2] = Q[2] + ex * ez;
            Q[3] = Q[3] + ey * ey, Q[4] = Q[4] + ey * ez, Q[5] = Q[5] + ez * ez;
        }
        flipped[i] = rtr::normal_fit(S, Q, found[i] + 1u, p, with_view != 0, view, &normals[i * 3], &curv[i]) ? 1 : 0;
    }
    f = fopen(out_path, "wb");
    if (!f || fwrite(normals.data(), 4, n * 3, f) != n * 3 || fwrite(curv.data(), 4, n, f) != n || fwrite(flipped.data(), 1, n, f) != n) return 2;
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 60;
    unsigned long cases = 0;
    if (rows(trials, &cases)) return 1;
    // a few roots whatever the input: exact squares, their neighbours, the ends of the range
    for (double x : {0.0, 1.0, 2.0, 4.0, 1.0 + 0x1p-52, 1.0 - 0x1p-53, 0x1p-1022, 0x1p-1074, 1.7976931348623157e308, (double)INFINITY, 3.0, 1e-300, 0.1})
        (void)rtr::sqrt_rn(x);
    if (argc > 3)
        if (int rc = fit(argv[2], argv[3])) return rc;
    if (g_fixed) { fprintf(stderr, "sqrt_rn changed the host's sqrt for %lu of %lu arguments\n", g_fixed, g_roots); return 1; }
    printf("%lu cases, %d trials per k, %lu square roots\n", cases, trials, g_roots);
    return 0;
}
