// The merge rule of the blockwise k-nearest-neighbour search (nn.rs:38-83 asks for the k nearest, `exhaustive_knn`,
// nn.rs:112-137, orders them as (distance, index) tuples), written once for host and device: the same source runs in
// knn_merge_kernel of knn.hip and behind scanrs_host_knn_merge, which the CPU test-suite checks against its numpy model.
//
// A list is k entries of (squared distance, global index), ascending in that order, padded at the end with (+inf, UINT32_MAX).
// Two lists whose real entries share no index merge into the k smallest of their union, again padded. Nothing here is
// order-dependent: every entry computes its own place from two binary searches, so any number of threads may place any entries.
#pragma once
#include <cstdint>

#ifndef SCANRS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCANRS_HD __host__ __device__
#else
#define SCANRS_HD
#endif
#endif

namespace scanrs {
namespace knn_merge {

// the total order of the search: the smaller squared distance first, equal distances by ascending global index
SCANRS_HD inline bool before(double da, uint32_t ia, double db, uint32_t ib) { return da < db || (da == db && ia < ib); }

// how many entries of the sorted list come before (x, xi); or_equal: an entry equal to it (padding meets padding) counts too
SCANRS_HD inline uint32_t rank_in(const double *d, const uint32_t *i, uint32_t k, double x, uint32_t xi, bool or_equal) {
    uint32_t lo = 0, hi = k;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (before(d[mid], i[mid], x, xi) || (or_equal && d[mid] == x && i[mid] == xi))
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

// Entry e of the 2k entries (e < k: entry e of list a, otherwise entry e - k of list b) goes to its place of the merged order when
// that place is among the first k. On a tie list a goes first: only padding ties, and the padding of b then lands behind the end.
SCANRS_HD inline void place(uint32_t k, const double *da, const uint32_t *ia, const double *db, const uint32_t *ib, uint32_t e, double *dout,
                            uint32_t *iout) {
    const bool from_a = e < k;
    const uint32_t j = from_a ? e : e - k;
    const double x = from_a ? da[j] : db[j];
    const uint32_t xi = from_a ? ia[j] : ib[j];
    const uint32_t pos = j + (from_a ? rank_in(db, ib, k, x, xi, false) : rank_in(da, ia, k, x, xi, true));
    if (pos < k) {
        dout[pos] = x;
        iout[pos] = xi;
    }
}

} // namespace knn_merge
} // namespace scanrs
