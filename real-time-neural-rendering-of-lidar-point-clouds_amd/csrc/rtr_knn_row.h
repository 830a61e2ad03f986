// rtr_knn_row.h -- the row of the k smallest squared distances that a query point of rtr_select_statistical keeps
// (include/rtr_statistics.h section 6n), free of HIP apart from the qualifiers: the kernel (rtr_statistical.hip, k_nb_rows)
// runs it over a row in LDS, tests/cpp/knn_row_check.cpp over a plain array with g++.
//
// A Row is anything with  float get(uint32_t slot) const  and  void set(uint32_t slot, float v)  over at least k slots.
// The values are squared distances: finite, >= +0, never -0 and never NaN, so the float comparisons below order them as
// their bits do.  The row is an unordered multiset while it is filled:
//   * a value enters a row that is not full in the next free slot;
//   * a full row takes a value only when it is SMALLER than the row's worst (largest) value, in the worst value's slot,
//     and is then scanned once for its new worst.  A value equal to the worst is dropped: it would change nothing in the
//     multiset of the k smallest.
// The worst value and its slot live in the state (registers), so a value that does not enter costs one comparison and
// no access to the row.  knn_row_sort puts the row in ascending order (insertion sort: the row is short and lives where
// one lane reaches it alone); knn_row_mean is the contract's fp32 sum of square roots, in that order, and its division.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTR_KNN_HD __host__ __device__ __forceinline__
#else
#define RTR_KNN_HD inline
#endif

namespace rtr {

struct KnnRowState {
    uint32_t count = 0;       // the filled slots: 0 .. k
    uint32_t worst_slot = 0;  // the slot of the largest value among them (any one of equals)
    float worst = 0.f;        // ... and that value
};

// d2 into the row of k (>= 1) slots; true when the row was written
template <class Row> RTR_KNN_HD bool knn_row_insert(Row &row, uint32_t k, KnnRowState &st, float d2) {
    if (st.count < k) {
        row.set(st.count, d2);
        if (st.count == 0u || d2 > st.worst) st.worst = d2, st.worst_slot = st.count;
        ++st.count;
        return true;
    }
    if (!(d2 < st.worst)) return false;
    row.set(st.worst_slot, d2);
    float w = row.get(0);
    uint32_t ws = 0;
    for (uint32_t s = 1; s < k; ++s) {
        const float v = row.get(s);
        if (v > w) w = v, ws = s;
    }
    st.worst = w, st.worst_slot = ws;
    return true;
}

// the first `count` slots into ascending order
template <class Row> RTR_KNN_HD void knn_row_sort(Row &row, uint32_t count) {
    for (uint32_t i = 1; i < count; ++i) {
        const float v = row.get(i);
        uint32_t j = i;
        for (; j > 0; --j) {
            const float below = row.get(j - 1);
            if (!(below > v)) break;
            row.set(j, below);
        }
        if (j != i) row.set(j, v);
    }
}

// The mean distance of a SORTED row: s = s + sqrtf(d2) slot by slot, every square root and every sum rounded to fp32 on
// its own, then one fp32 division by the count; +inf for an empty row.
template <class Row> RTR_KNN_HD float knn_row_mean(const Row &row, uint32_t count) {
    if (count == 0u) return INFINITY;
    float s = 0.f;
    for (uint32_t i = 0; i < count; ++i) s = s + sqrtf(row.get(i));
    return s / (float)count;
}

}  // namespace rtr
