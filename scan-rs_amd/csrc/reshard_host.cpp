// reshard_host.cpp — the plan of the inner-sharding constructors on host arrays (scanrs_host_plan_inner): what the
// device path of multi.cpp / reshard.hip is checked against. No device is touched.
#include <algorithm>

#include "common.hpp"

namespace scanrs {

// scanrs_mat_create's checks of a triplet's frame, shared by the constructors and the host plan (same codes, same messages)
void reshard_check_frame(uint64_t n_outer, uint64_t n_inner, const uint64_t *indptr, const uint32_t *indices, bool values_given) {
    if (!indptr) fail(SCANRS_ERR_ARGUMENT, "null indptr");
    if (n_outer > 0xFFFFFFFFull || n_inner > 0xFFFFFFFFull) fail(SCANRS_ERR_SHAPE, "dimensions must fit in u32 (AdaptiveVec limit)");
    if (indptr[0] != 0) fail(SCANRS_ERR_ARGUMENT, "indptr[0] must be 0");
    // the slabs are cut from indptr on the host before any of it reaches a device: it must not decrease
    unsigned long long bad = 0;
    for (uint64_t o = 0; o < n_outer; o++) bad += indptr[o + 1] < indptr[o];
    if (bad) fail(SCANRS_ERR_ARGUMENT, "indices must be in range and strictly ascending within each outer vector (%llu violations)", bad);
    if (indptr[n_outer] && (!indices || !values_given)) fail(SCANRS_ERR_ARGUMENT, "null indices/values");
}

void reshard_host_plan(const uint64_t *indptr, const uint32_t *indices, uint64_t n_outer, uint64_t n_inner, uint32_t world, uint64_t *slab_bounds,
                       uint64_t *bounds, uint64_t *moved) {
    if (world == 0) fail(SCANRS_ERR_ARGUMENT, "world must be at least 1");
    reshard_check_frame(n_outer, n_inner, indptr, indices, true);
    unsigned long long bad = 0;
    std::vector<uint64_t> tip(n_inner + 1, 0); // the transposed indptr: stored entries per inner position, zeros included
    for (uint64_t o = 0; o < n_outer; o++)
        for (uint64_t p = indptr[o]; p < indptr[o + 1]; p++) {
            const uint32_t j = indices[p];
            if ((uint64_t)j >= n_inner)
                bad++;
            else
                tip[j + 1]++;
            if (p > indptr[o] && j <= indices[p - 1]) bad++;
        }
    if (bad) fail(SCANRS_ERR_ARGUMENT, "indices must be in range and strictly ascending within each outer vector (%llu violations)", bad);
    for (uint64_t j = 0; j < n_inner; j++) tip[j + 1] += tip[j];
    std::vector<uint64_t> sb(world + 1), bd(world + 1);
    if (scanrs_plan_shards(indptr, n_outer, world, sb.data()) != SCANRS_OK || scanrs_plan_shards(tip.data(), n_inner, world, bd.data()) != SCANRS_OK)
        throw Failure{SCANRS_ERR_ARGUMENT};
    if (slab_bounds) std::copy(sb.begin(), sb.end(), slab_bounds);
    if (bounds) std::copy(bd.begin(), bd.end(), bounds);
    if (!moved) return;
    std::fill(moved, moved + (size_t)world * world, 0ull);
    for (uint32_t s = 0; s < world; s++)
        for (uint64_t o = sb[s]; o < sb[s + 1]; o++)
            for (uint64_t p = indptr[o]; p < indptr[o + 1]; p++) {
                // the shard whose range holds the index: the last d with bounds[d] <= j (empty ranges repeat a bound)
                const uint32_t d = (uint32_t)(std::upper_bound(bd.begin() + 1, bd.end() - 1, (uint64_t)indices[p]) - (bd.begin() + 1));
                moved[(size_t)s * world + d]++;
            }
}

} // namespace scanrs

using namespace scanrs;

extern "C" int scanrs_host_plan_inner(const uint64_t *indptr, const uint32_t *indices, uint64_t n_outer, uint64_t n_inner, uint32_t world,
                                      uint64_t *slab_bounds, uint64_t *bounds, uint64_t *moved) {
    return guard([&] { reshard_host_plan(indptr, indices, n_outer, n_inner, world, slab_bounds, bounds, moved); });
}
