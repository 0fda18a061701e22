// The exchange steps of one operation over a (possibly unsharded) handle ("The exchange layer"): the counted u64
// all-reduce, and the gather of a few words per rank that is built on it. Bound to the handle and to the counter the operation
// reports (scanrs_mat_get_counter), e.g. ShardExchange{st, st.de_shard_allreduces}.
#pragma once
#include "common.hpp"

#include <vector>

namespace scanrs {

struct ShardExchange {
    Storage &st;
    uint64_t &steps;
    bool active() const { return st.shard.active(); }
    // One step on st.stream, counted; nothing on an unsharded handle. The count is not looked at: a collective must not depend on
    // what one rank sees, so a caller whose count can be 0 (on every rank alike) tests it itself, in front of the call.
    void sum(unsigned long long *d, uint64_t count) {
        if (!active()) return;
        allreduce_u64(st, d, count);
        steps++;
    }
    // The transport only sums. What has to be maximised, minimised or compared across the ranks travels in the rank's own slot of a
    // zeroed array instead: rank r's `per_rank` (>= 1) words come back as the words [r * per_rank, (r + 1) * per_rank) of the result,
    // the same on every rank, in ONE step (also at world == 1 with a transport). An unsharded handle gets its own words back. The
    // result is on the host when the call returns. `gather` reads device memory and waits for nothing before the step; `gather_host`
    // reads host memory, which may be pageable and may go out of use right after the call.
    std::vector<unsigned long long> gather(const unsigned long long *d_mine, uint64_t per_rank) { return gather_from(d_mine, per_rank, false); }
    std::vector<unsigned long long> gather_host(const unsigned long long *h_mine, uint64_t per_rank) { return gather_from(h_mine, per_rank, true); }

  private:
    std::vector<unsigned long long> gather_from(const unsigned long long *mine, uint64_t per_rank, bool on_host); // capi.cpp
};

} // namespace scanrs
