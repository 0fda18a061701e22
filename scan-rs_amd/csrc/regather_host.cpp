// regather_host.cpp — the plan of scanrs_multi_gather_outer / scanrs_multi_rebalance on host arrays (scanrs_host_plan_gather;
// DESIGN §7n). The device path of multi.cpp runs this very function on the indptr it assembled from the source shards, so the plan
// a test reads back (scanrs_multi_gather_info) and the plan it computes here are the same code. No device is touched.
#include <algorithm>

#include "common.hpp"

namespace scanrs {

// the refusals of a list along the outer dimension, in select_outer's words (select_host.cpp)
void regather_check_list(const uint64_t *idx, uint64_t n_idx, uint64_t n_outer) {
    if (n_idx && !idx) fail(SCANRS_ERR_ARGUMENT, "idx: null index list");
    if (n_idx >= 0x7FFFFFFFull) fail(SCANRS_ERR_SHAPE, "idx: the result needs dimensions below 2^31 - 1 (%llu entries)", (unsigned long long)n_idx);
    for (uint64_t i = 0; i < n_idx; i++)
        if (idx[i] >= n_outer)
            fail(SCANRS_ERR_INVALID, "idx: index out of range: entry %llu of the list is %llu, the matrix has %llu outer vectors", (unsigned long long)i,
                 (unsigned long long)idx[i], (unsigned long long)n_outer);
}

void regather_host_plan(const uint64_t *indptr, uint64_t n_outer, const uint64_t *src_bounds, uint32_t n_src, const uint64_t *idx, uint64_t n_idx,
                        uint32_t n_dst, uint64_t *out_indptr, uint64_t *bounds, uint64_t *moved) {
    if (!indptr) fail(SCANRS_ERR_ARGUMENT, "null indptr");
    if (!src_bounds) fail(SCANRS_ERR_ARGUMENT, "src_bounds: null source bounds");
    if (n_src == 0 || n_src > REGATHER_MAX_SHARDS) fail(SCANRS_ERR_ARGUMENT, "n_src: 1 <= n_src <= 16 is required");
    if (n_dst == 0 || n_dst > REGATHER_MAX_SHARDS) fail(SCANRS_ERR_ARGUMENT, "n_shards: 1 <= n_shards <= 16 is required");
    if (src_bounds[0] != 0 || src_bounds[n_src] != n_outer) fail(SCANRS_ERR_ARGUMENT, "src_bounds: the source bounds must run from 0 to the outer extent");
    for (uint32_t s = 0; s < n_src; s++)
        if (src_bounds[s + 1] < src_bounds[s]) fail(SCANRS_ERR_ARGUMENT, "src_bounds: the source bounds must not descend");
    for (uint64_t o = 0; o < n_outer; o++)
        if (indptr[o + 1] < indptr[o]) fail(SCANRS_ERR_ARGUMENT, "indptr must not descend");
    regather_check_list(idx, n_idx, n_outer);
    // T's indptr: the prefix sum of the listed vectors' lengths
    std::vector<uint64_t> tip(n_idx + 1, 0);
    for (uint64_t j = 0; j < n_idx; j++) tip[j + 1] = tip[j] + (indptr[idx[j] + 1] - indptr[idx[j]]);
    std::vector<uint64_t> bd(n_dst + 1);
    if (scanrs_plan_shards(tip.data(), n_idx, n_dst, bd.data()) != SCANRS_OK) throw Failure{SCANRS_ERR_ARGUMENT};
    if (out_indptr) std::copy(tip.begin(), tip.end(), out_indptr);
    if (bounds) std::copy(bd.begin(), bd.end(), bounds);
    if (!moved) return;
    std::fill(moved, moved + (size_t)n_src * n_dst, 0ull);
    for (uint32_t d = 0; d < n_dst; d++)
        for (uint64_t j = bd[d]; j < bd[d + 1]; j++) {
            // the source shard whose range holds the vector: the last s with src_bounds[s] <= idx[j] (empty ranges repeat a bound)
            const uint32_t s = (uint32_t)(std::upper_bound(src_bounds + 1, src_bounds + n_src, idx[j]) - (src_bounds + 1));
            moved[(size_t)s * n_dst + d] += tip[j + 1] - tip[j];
        }
}

} // namespace scanrs

using namespace scanrs;

extern "C" int scanrs_host_plan_gather(const uint64_t *indptr, uint64_t n_outer, const uint64_t *src_bounds, uint32_t n_src, const uint64_t *idx,
                                       uint64_t n_idx, uint32_t n_dst, uint64_t *out_indptr, uint64_t *bounds, uint64_t *moved) {
    return guard([&] { regather_host_plan(indptr, n_outer, src_bounds, n_src, idx, n_idx, n_dst, out_indptr, bounds, moved); });
}
