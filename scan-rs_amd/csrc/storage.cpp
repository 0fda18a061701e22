// What a handle's storage owns beyond its arrays: the per-kernel-class profile, the helper thread of the side build, the lazily
// created streams, and the destructor that drains them.
#include "common.hpp"

namespace scanrs {

// ---- Profile -----------------------------------------------------------------------------------
hipEvent_t Profile::take() {
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e;
    SCANRS_HIP(hipEventCreate(&e));
    return e;
}
void Profile::begin(hipStream_t s, const char *name, double bytes, double onchip) {
    Rec r{name, take(), take(), bytes, onchip};
    SCANRS_HIP(hipEventRecord(r.a, s));
    pending.push_back(r);
}
void Profile::end(hipStream_t s) {
    if (pending.empty()) return;
    (void)hipEventRecord(pending.back().b, s);
}
void Profile::resolve() {
    for (auto &r : pending) {
        float ms = 0.f;
        if (wait_event_quiet(r.b) && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            auto &st = stats[r.name];
            st.launches++;
            st.ms += ms;
            st.bytes += r.bytes;
            st.onchip += r.onchip;
        }
        pool.push_back(r.a);
        pool.push_back(r.b);
    }
    pending.clear();
}
void Profile::reset() {
    resolve();
    stats.clear();
}
Profile::~Profile() {
    for (auto &r : pending) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto e : pool) (void)hipEventDestroy(e);
}

// Waits until the helper has finished with `target` (nullptr: with everything) and rethrows its failure. `need_layout` false: the
// copy itself is enough (a reader of the triplet).
void Storage::side_join_if(const SparseCopy *target, bool need_layout) {
    if (!side) return;
    SideBuild *sb = side;
    const auto t0 = std::chrono::steady_clock::now();
    bool all = target == nullptr;
    {
        std::unique_lock<std::mutex> lk(sb->mu);
        if (target) {
            int pos = sb->order[0] == target ? 0 : sb->order[1] == target ? 1 : -1;
            if (pos < 0) return; // the helper does not touch this copy
            const double dl = sync_timeout_s() * 4.0; // builds are many device waits long; each of them is bounded by itself
            const bool ok = sb->cv.wait_for(lk, std::chrono::duration<double>(dl), [&] {
                return sb->finished || sb->code != SCANRS_OK || (need_layout ? sb->layout_done[pos] : sb->copy_done[pos]);
            });
            if (!ok) fail(SCANRS_ERR_DEVICE, "the helper thread that builds the second orientation did not finish a stage within %.0f s", dl);
            all = sb->finished || sb->code != SCANRS_OK;
        }
    }
    if (all) { // the helper is done (or failed): take it down
        registry_set_side(*this, nullptr);
        if (sb->th.joinable()) sb->th.join();
        if (sb->stream) (void)hipStreamDestroy(sb->stream);
        const int code = sb->code;
        const std::string err = sb->err;
        if (trace_on()) fprintf(stderr, "[scanrs trace] side build: %.3f ms on the helper thread\n", sb->ms);
        delete sb;
        t_side_wait_us += (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (code != SCANRS_OK && std::uncaught_exceptions() == 0) fail(code, "%s", err.c_str());
        return;
    }
    t_side_wait_us += (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}
Storage::~Storage() {
    RegistryLeave leave(this); // out of the set of handles FIRST; while this destructor drains the streams the process counts as busy
    if (side) {
        try {
            side_join_if(nullptr, true);
        } catch (const Failure &) {
        }
    }
    if (host_stage) pinned_give(host_stage, host_stage_bytes);
    auto drain = [](hipStream_t s) { (void)wait_stream_quiet(s), (void)hipStreamDestroy(s); }; // each stream drained before it goes
    for_each_stream(*this, [&](const char *, hipStream_t s) { if (s != stream) drain(s); }); // (the helper's went with the helper; main goes last)
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_ov) (void)hipEventDestroy(ev_ov);
    if (stream) drain(stream);
}
// Four streams per handle: the main stream (sparse products: the persistent tile kernel must get its CUs first) at the default
// priority, the overflow gather (fills the registers the tile kernel leaves) and the two auxiliary streams (dense work nothing
// waits for until the end of the iterations) at the lowest.
static int stream_priority(int level) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest); // numerically greatest <= least
    (void)level;
    return least;
}
hipStream_t Storage::aux() {
    if (!opt.overlap) return stream;
    if (!aux_stream) {
        // lowest priority: at the end of a persistent tile kernel the NEXT one (main stream) gets the CUs first and this stream's
        // dense kernels fill what its tail and the overflow gather's tail leave — at equal priority a 2-3 ms projection GEMM that
        // became runnable at the same moment held the next sparse product back by its whole duration
        SCANRS_HIP(hipStreamCreateWithPriority(&aux_stream, hipStreamDefault, stream_priority(2)));
    }
    return aux_stream;
}
hipStream_t Storage::aux2() {
    if (!opt.overlap) return stream;
    if (!aux2_stream) SCANRS_HIP(hipStreamCreateWithPriority(&aux2_stream, hipStreamDefault, stream_priority(2)));
    return aux2_stream;
}
hipStream_t Storage::ov() {
    if (!ov_stream) {
        // lowest priority: the persistent tile kernel's workgroups are placed first, the gather fills what is left of a CU
        SCANRS_HIP(hipStreamCreateWithPriority(&ov_stream, hipStreamNonBlocking, stream_priority(1)));
        SCANRS_HIP(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
        SCANRS_HIP(hipEventCreateWithFlags(&ev_ov, hipEventDisableTiming));
    }
    return ov_stream;
}
SparseCopy &Storage::copy_with_outer_rows(bool outer_rows) {
    const bool primary_outer_rows = storage == SCANRS_CSR;
    if (outer_rows == primary_outer_rows) return primary;
    side_join_if(&other, false); // a helper thread may be building it right now
    if (!has_other) {
        build_transposed_copy(*this, primary, other);
        has_other = true;
    }
    other_settled = true;
    return other;
}

} // namespace scanrs
