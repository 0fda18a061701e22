// Shared declarations of the scanrs_amd library (host side). gfx950 only.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <cstdio>
#include <cstdint>
#include <cstdarg>
#include <functional>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "scanrs_amd.h"
#include "common_err.hpp"
#include "options.hpp"

struct scanrs_comm; // comm.cpp

namespace scanrs {

#define SCANRS_HIP(expr)                                                                              \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            ::scanrs::fail(SCANRS_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                           __FILE__, __LINE__);                                                       \
    } while (0)

// SCANRS_TRACE=1: wall-clock of host-side phases on stderr (diagnostics only)
bool trace_on();
// Where the calling thread stands: kept in a small per-thread ring (always; a timed-out wait names the last ones) and printed with
// SCANRS_TRACE=2 (a line on stderr, no synchronisation)
void stage_mark(const char *what, long a = 0, long b = 0);

// ---- bounded waits ----------------------------------------------------------------------------------------------------
// Every host-side wait for the device goes through these: a poll (hipStreamQuery / hipEventQuery, spinning for the first
// 200 us, then short sleeps) with a deadline — option "sync_timeout_s", default 120 s — instead of a blocking
// hipStreamSynchronize / hipEventSynchronize: a device that never signals turns into SCANRS_ERR_DEVICE naming the wait
// (function, file:line), the thread's last stage marks and which of the handle's streams are still busy, not into a call that
// never returns. The *_quiet forms are for destructors and unwinding (bounded too, nothing thrown).
struct Storage;
void wait_stream(hipStream_t s, const char *func, const char *file, int line);
void wait_event(hipEvent_t e, const char *func, const char *file, int line);
void wait_device(const char *func, const char *file, int line);
bool wait_stream_quiet(hipStream_t s) noexcept;
bool wait_event_quiet(hipEvent_t e) noexcept;
double sync_timeout_s();
void set_sync_timeout_s(double s);
// the handle whose streams a timed-out wait on this thread reports (set by the entry points that run device work)
struct CurrentHandle {
    const Storage *prev;
    // Every entry point that queues device work makes one: after a timed-out wait (device_lost) it refuses until the device has been seen
    // idle again. `waits_only`: an entry point that only waits (scanrs_mat_sync) - the way to get there.
    explicit CurrentHandle(const Storage *st, bool waits_only = false);
    ~CurrentHandle();
};
#define SCANRS_LOCAL __attribute__((visibility("hidden"))) // shared between the library's own files, not an exported symbol
SCANRS_LOCAL const Storage *current_handle(); // what the innermost CurrentHandle of this thread holds (nullptr: none)
// scanrs_mat_free: the storage whose members are being destroyed on this thread (its streams are drained by its destructor)
struct SCANRS_LOCAL DyingHandle {
    explicit DyingHandle(const Storage *st);
    ~DyingHandle();
};
SCANRS_LOCAL const Storage *dying_handle();
SCANRS_LOCAL bool device_ok();        // a gfx950 device is usable from this process
SCANRS_LOCAL bool device_recovered(); // after a timed-out wait: has the whole device been seen idle again? (clears device_lost)
SCANRS_LOCAL void need_device();      // fails unless device_ok() and device_recovered()
// The handles of this process (runtime.cpp). A handle leaves FIRST in its destructor; while its RegistryLeave lives the process counts as busy.
SCANRS_LOCAL void registry_add(const Storage *st);
struct SCANRS_LOCAL RegistryLeave {
    explicit RegistryLeave(const Storage *st);
    ~RegistryLeave();
};
SCANRS_LOCAL bool all_library_streams_idle();
SCANRS_LOCAL bool wait_all_idle_quiet() noexcept; // the null stream and every library stream idle within the deadline (polled, nothing thrown)

template <typename F>
static int guard(F &&f) {
    try {
        f();
        return SCANRS_OK;
    } catch (const Failure &e) {
        return e.code;
    } catch (const std::bad_alloc &) {
        set_error("out of host memory");
        return SCANRS_ERR_DEVICE;
    } catch (const std::exception &e) {
        set_error("internal error: %s", e.what());
        return SCANRS_ERR_DEVICE;
    }
}
#define SCANRS_SYNC(stream) ::scanrs::wait_stream((stream), __PRETTY_FUNCTION__, __FILE__, __LINE__)
// A few bytes from the device whose landing place outlives a timed-out wait (copies into stack variables of a frame that a
// timeout unwinds would land in whatever lives there later): the copy goes into a slot of a process-wide pinned ring and is read from
// there behind the wait; when the wait gives up, the slot is simply not read.
void *landing_slot(size_t bytes); // runtime.cpp: 8-byte aligned, from a pinned ring of 1 MB that is never unmapped
// Device -> host for arrays: through a pinned staging area that is never unmapped, in pieces of at most 8 MB, each piece waited for
// (bounded) before it is copied on into `dst`. If a wait gives up, the copy still in flight lands in the staging area — not in a
// vector or a caller's array whose frame has unwound meanwhile. `src_pitch` / `row_bytes` / `rows`: a 2-D copy into a
// compact destination.
void d2h_landed(void *dst, const void *dsrc, size_t bytes, hipStream_t s, const char *func, const char *file, int line);
void d2h_landed_2d(void *dst, const void *dsrc, size_t src_pitch, size_t row_bytes, size_t rows, hipStream_t s, const char *func, const char *file, int line);
#define SCANRS_D2H(dst, dsrc, bytes, stream) ::scanrs::d2h_landed((dst), (dsrc), (bytes), (stream), __PRETTY_FUNCTION__, __FILE__, __LINE__)
#define SCANRS_D2H_2D(dst, dsrc, pitch, row_bytes, rows, stream) ::scanrs::d2h_landed_2d((dst), (dsrc), (pitch), (row_bytes), (rows), (stream), __PRETTY_FUNCTION__, __FILE__, __LINE__)
template <typename T>
inline T d2h_value(const T *d, hipStream_t s, const char *func, const char *file, int line) {
    T *slot = static_cast<T *>(landing_slot(sizeof(T)));
    const hipError_t e = hipMemcpyAsync(slot, d, sizeof(T), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) ::scanrs::fail(SCANRS_ERR_DEVICE, "hipMemcpyAsync failed: %s (%s:%d)", hipGetErrorString(e), file, line);
    wait_stream(s, func, file, line);
    return *slot;
}
#define SCANRS_D2H_VALUE(dptr, stream) ::scanrs::d2h_value((dptr), (stream), __PRETTY_FUNCTION__, __FILE__, __LINE__)
#define SCANRS_SYNC_EVENT(ev) ::scanrs::wait_event((ev), __PRETTY_FUNCTION__, __FILE__, __LINE__)
struct Tick {
    const char *what;
    std::chrono::steady_clock::time_point t0;
    explicit Tick(const char *w) : what(w), t0(std::chrono::steady_clock::now()) {}
    ~Tick() {
        if (trace_on())
            fprintf(stderr, "[scanrs trace] %-28s %8.3f ms\n", what,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

// ---- device memory ------------------------------------------------------------------
// hipFree waits for the whole device (a buffer dropped while a 20 ms sparse pass runs holds the host for those 20 ms), and VRAM
// that was just freed is scrubbed in the background: an allocation right behind a large free waits for the scrubber (0.24 s
// per 8 GB, profiles/microbench/alloc_probe2). So buffers are never freed in the middle of a call: release() hands the pointer
// to a list, together with one event per stream of the releasing handle; a block whose events have completed joins the cache at the
// next allocation, and goes back to the driver only where a call ends (end of create / a solver / scanrs_mat_sync / scanrs_mat_free)
// or when an allocation fails for lack of memory, which then tries again.
void device_free_later(void *p, size_t bytes);
void device_free_flush() noexcept;                             // released blocks whose release events have completed
void device_free_flush_owner_gone(const void *owner) noexcept; // blocks of a handle that has just been destroyed
bool device_lost();                                            // a bounded wait gave up earlier: nothing is reused or freed, entry points fail fast
void *device_alloc(size_t bytes); // hipMalloc with the retry above; throws Failure(SCANRS_ERR_DEVICE)
void device_cache_release() noexcept;
void device_reserve(size_t bytes);
void device_cache_set_fraction(double f);
size_t device_cache_bytes();
size_t device_live_bytes();
size_t device_reserve_unused_bytes();
SCANRS_LOCAL void device_memory_report(const char *why); // SCANRS_TRACE: what the library holds on the device, block by block, on stderr
SCANRS_LOCAL void reserve_selftest(uint32_t rounds, uint64_t seed); // scanrs_debug_arena_selftest (device_memory.cpp: the arena's take / give, no device)
void library_warm_up(); // kernels.hip: loads every code object of the library (one empty launch per translation unit)
uint64_t device_alloc_us();
uint64_t device_alloc_calls();

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    explicit DevBuf(size_t count) { alloc(count); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            n = o.n;
            o.p = nullptr;
            o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    static constexpr size_t SLACK = 4096;
    void alloc(size_t count) {
        release();
        n = count;
        if (!count) return;
        // Slack behind every buffer: kernels that read a vector in aligned 16-byte chunks (tile_assign_wave_kernel) look up to two
        // chunks past the end of the last vector; the tile kernel loads the records and weights of the next two visits without
        // asking whether they exist (spmm_tile_body: 2 visits x 2 sets x 64 weights x 8 B behind the last group's last visit)
        p = static_cast<T *>(device_alloc(count * sizeof(T) + SLACK));
    }
    void ensure(size_t count) {
        if (count > n) alloc(count);
    }
    void release() {
        if (p) device_free_later(p, n * sizeof(T) + SLACK);
        p = nullptr;
        n = 0;
    }
};

// Grow-only named scratch buffers: nothing is hipMalloc'ed inside the solver loops after
// the first pass over them.
struct Scratch {
    std::map<std::string, DevBuf<char>> bufs;
    hipStream_t stream = nullptr; // zero-fills are ordered on the owning handle's stream
    template <typename T>
    T *get(const std::string &key, size_t count) {
        auto &b = bufs[key];
        size_t bytes = count * sizeof(T);
        if (bytes > b.n) {
            // (an eighth more, so that a slightly larger request does not reallocate - up to 32 MB (uncapped, the two 30 GB projection panels of a
            // PCA of a 3.75 M-cell shard carried 7.5 GB of it))
            b.alloc(bytes + std::min<size_t>(bytes / 8, (size_t)32 << 20) + 256);
            SCANRS_HIP(hipMemsetAsync(b.p, 0, b.n, stream)); // padding columns of panels start out as zeros
        }
        return reinterpret_cast<T *>(b.p);
    }
    std::set<std::string> filled; // keys whose (constant) contents are already on the device
    void clear() {
        bufs.clear();
        filled.clear();
    }
};

// ---- per-kernel-class timing (scanrs_profile_*) -------------------------------------
struct Profile {
    bool on = false;
    struct Rec {
        std::string name;
        hipEvent_t a, b;
        double bytes, onchip;
    };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    struct Stat {
        uint64_t launches = 0;
        double ms = 0, bytes = 0, onchip = 0;
    };
    std::map<std::string, Stat> stats;
    hipEvent_t take();
    void begin(hipStream_t s, const char *name, double bytes, double onchip = 0.0);
    void end(hipStream_t s);
    void resolve();
    void reset();
    ~Profile();
};

// ---- sparse storage -------------------------------------------------------------------
// One wave works one item: a run of at most ITEM_NNZ nonzeros of one outer vector.
// Outer vectors longer than that are cut into several items whose partial results go
// through a slab and are summed in item order (deterministic, no float atomics).
constexpr uint32_t ITEM_NNZ = 8192;
constexpr uint32_t NO_SLAB = 0xFFFFFFFFu;

struct Item {
    uint64_t start; // offset of the first nonzero in indices/values
    uint32_t row;   // outer vector id
    uint32_t len;   // number of nonzeros
    uint32_t slab;  // slab row for the partial result, NO_SLAB when the item is the whole vector
    uint32_t _pad;
};

struct MultiRow {
    uint32_t row;
    uint32_t first_slab;
    uint32_t count;
    uint32_t _pad;
};

// tiles.hip: the split of an orientation (under one map) into fixed record positions per (outer vector, panel tile) and an
// overflow matrix — what the hybrid LDS-tile + gather product walks
struct TileLayout;
void tile_layout_free(TileLayout *t);
void tile_layout_forget_weights(TileLayout *t);
void tile_layout_stats(const TileLayout *t, uint64_t out[3]); // positions per pass, served nonzeros, overflow nonzeros

// A compressed orientation: n_outer vectors over n_inner positions. The three arrays are DevBuf allocations of their own: each starts
// on (at least) a 16-byte boundary and has DevBuf::SLACK readable bytes behind its last entry. select.hip and encode.hip rely on both
// (16-byte loads that begin at a multiple of 4 / 8 entries and may run past nnz); a copy around borrowed or offset pointers would
// have to keep them.
struct SparseCopy {
    uint64_t n_outer = 0, n_inner = 0, nnz = 0;
    DevBuf<uint64_t> indptr;
    DevBuf<uint32_t> indices, values;
    DevBuf<Item> items;
    DevBuf<MultiRow> multi;
    uint32_t n_items = 0, n_multi = 0, n_slab = 0;
    uint32_t max_value = 0;  // largest count (0: not computed yet; counts are >= 1) — bound of the mapped values for col_moments_kernel
    DevBuf<uint32_t> bounds; // L2-blocked gather: offset of the first nonzero >= b*1024 within each outer vector
    // L2-blocked gather, launch order: outer vectors by descending length (longest first) and the sorted lengths
    // on the host (how many vectors are "hot" for a given step count is a binary search)
    DevBuf<uint32_t> order;
    std::vector<uint32_t> sorted_len;
    std::shared_ptr<TileLayout> tiles; // built on first use of the hybrid tile product under a given map (tiles.hip)
    uint64_t tile_rejected_shape = 0;  // the tile shape (and overflow limit) whose layout was not worth building for this copy (0: none)
    int tsig_n = -1;                   // ... the map the last eligible product came with (auto path: build on the second sighting)
    uint32_t tsig_id[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int tsig_outer[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // Materialized map values (kernels.hip, "materialized prefix"): f64 per nonzero, in this copy's order, of the first
    // `fsig_n` links of a map chain — kept for the copy with few, long outer vectors, where evaluating the chain costs a
    // scattered 8-byte gather per nonzero per product (the per-barcode scale while walking a gene's vector).
    DevBuf<double> fvals;
    int fsig_n = 0;
    uint32_t fsig_id[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // MapOp ids of the materialized links (never reused)
    int fsig_outer[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // ... and how each indexes its arrays in this copy
    void build_items(hipStream_t s);
};

struct ShardInfo {
    uint32_t rank = 0, world = 1;
    uint64_t outer_begin = 0, outer_global = 0;
    scanrs_allreduce_fn allreduce = nullptr; // host-supplied hook (tests; a caller with its own transport)
    void *ctx = nullptr;
    scanrs_comm *comm = nullptr; // the library's own transport (RCCL or the single-process group); not owned
    // a transport given at world == 1 is still served (single-rank RCCL runs exercise the exchange steps)
    bool active() const { return world > 1 || allreduce != nullptr || comm != nullptr; }
};

// Storage shared by a handle and its views (AdaptiveMat::view / t share `&[AdaptiveVec]`).
// Pinned host staging buffers, kept across handles (device_memory.cpp): take the smallest idle one of at least `bytes` or pin a new one.
void *pinned_take(size_t bytes, size_t *got);
void pinned_give(void *p, size_t bytes) noexcept;

struct Storage {
    uint64_t rows = 0, cols = 0;
    int storage = SCANRS_CSR; // orientation of `primary`: CSR -> outer = rows
    SparseCopy primary;
    SparseCopy other; // the transposed orientation, built on first use
    std::atomic<bool> has_other{false}; // written by the helper thread too (SideBuild); readers that must not depend on its timing use other_settled
    bool other_settled = false;         // calling thread only: `other` is known to exist at a point of the program that does not depend on the helper's speed (copy_with_outer_rows)
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr; // small dense work that overlaps a sparse pass (svd_bk's cross-block orthogonalisation)
    hipStream_t aux();
    hipStream_t aux2_stream = nullptr; // svd_bk's early projection GEMMs (bulk work nothing waits for until the end of the iterations)
    hipStream_t aux2();
    // scratch key of the stream work is being queued on: the auxiliary stream runs beside the main one and must not share its temporaries
    std::string skey(const char *k) const {
        if (aux_stream && stream == aux_stream) return std::string(k) + "@aux";
        if (aux2_stream && stream == aux2_stream) return std::string(k) + "@aux2";
        return std::string(k);
    }
    hipStream_t ov_stream = nullptr; // the gather over the overflow part of a tile layout runs here, beside the tile kernel (tiles.hip)
    hipEvent_t ev_in = nullptr, ev_ov = nullptr;
    hipStream_t ov();
    // Side build (round 4): the copy and the tile layout that the SECOND product of a solver needs are made by a helper thread on a
    // stream of its own while the main thread prepares and runs the first product (capi.cpp, prepare_second_orientation)
    struct SideBuild;
    SideBuild *side = nullptr;
    void side_join_if(const SparseCopy *target, bool need_layout); // waits until the helper is done with `target` (its copy, or also its layout; nullptr: with everything); rethrows its failure
    uint64_t t_side_wait_us = 0, t_layout_us = 0, t_start_panel_us = 0, t_delivery_us = 0; // first-call accounting (scanrs_mat_get_counter)
    Scratch scratch;
    // GF(2) jump tables of the device-side seeded-panel generator (solver.cpp / omega_jump_kernel)
    DevBuf<uint64_t> jump_tab;
    uint64_t jump_d = 0;
    int jump_npow = 0;
    // grow-only pinned host staging buffer (seeded start panels): no page faults, DMA-speed uploads
    void *host_stage = nullptr;
    size_t host_stage_bytes = 0;
    // (from / back to a small process-wide pool, device_memory.cpp: pinning 64 MB takes several ms, and scanrs_init can do it ahead of the first call)
    void *pinned(size_t bytes) {
        if (bytes > host_stage_bytes) {
            if (host_stage) pinned_give(host_stage, host_stage_bytes);
            host_stage = nullptr;
            host_stage_bytes = 0;
            host_stage = pinned_take(bytes, &host_stage_bytes);
        }
        return host_stage;
    }
    Profile prof;
    ShardInfo shard; // sharding of primary's outer dimension
    // PcaResult of the last svd_bk / svd_rand call, as it lies in the solver's scratch (scanrs_pca_result_device)
    struct PcaDev {
        const double *u = nullptr, *v = nullptr;
        uint32_t ld_u = 0, ld_v = 0, k = 0;
        uint64_t rows_u = 0, rows_v = 0;
    } pca_dev;
    Options opt;                          // every knob of the handle (options.hpp; set through the table of options.cpp)
    const double *tile_xc_src = nullptr;  // the panel whose compact copy "tile_xc" already holds (set and cleared by mat_apply around one product)
    uint32_t tile_xc_l = 0;
    int tile_hint = 0;                    // > 0 while a solver that repeats the same products is running (svd_bk, svd_rand)
    uint64_t partition_allreduces = 0;    // exchange steps of the last scanrs_mat_partition_on_thresholds_sharded on this handle (an unsharded one: 0)
    uint64_t transpose_route = 0;         // the sort the last build_transposed_copy on this handle ran through: TransposeRoute of transpose_plan.hpp, 0 when none was built or it had no nonzeros (scanrs_mat_get_counter)
    uint64_t partition_rounds = 0;        // rounds of the last scanrs_mat_partition_on_thresholds on this handle, the final one that changes nothing included (scanrs_mat_get_counter)
    uint64_t de_shard_tests = 0, de_shard_allreduces = 0; // the last DE call on this handle: tests this rank launched on the device, exchange steps (scanrs_mat_get_counter)
    uint64_t de_pairs_passes = 0, de_pairs_literal = 0; // the last scanrs_sseq_de_pairs on this handle: passes over the nonzeros, pairs on the literal route (scanrs_mat_get_counter)
    uint64_t reshard_us[5] = {0, 0, 0, 0, 0}; // a shard of scanrs_multi_create_inner and kin: its thread's wall clock in upload, count, split, exchange, transpose (scanrs_mat_get_counter)
    uint64_t regather_us[3] = {0, 0, 0};  // a shard of scanrs_multi_gather_outer / _rebalance: wall clock of the plan (one phase of the calling thread, the same on every shard) and of its own thread in pull and finish (scanrs_mat_get_counter)
    uint64_t export_us[3] = {0, 0, 0};    // a shard of the last scanrs_multi_to_adaptive: wall clock of the plan (the transposed copies, their indptr to the host and the host plan: one phase, the same on every shard; 0 for major STORED) and of its own thread in pull (0 for STORED) and encode + download (scanrs_mat_get_counter)
    uint64_t subset_masked_passes = 0, subset_scatter_passes = 0; // sums over a column list made so far on this handle: from the copy whose outer dimension is the result axis / through the integer scatter (scanrs_mat_get_counter)
    uint64_t knn_blocks = 0, knn_allreduces = 0; // the last scanrs_knn_sharded / scanrs_nearest_neighbors_sharded on this handle: blocks of the point set searched, exchange steps (an unsharded one: 0)
    uint64_t knn_blocks_filtered = 0;     // the last scanrs_nearest_neighbors_sharded on this handle: blocks this rank searched through the filter (pearson / cosine)
    uint64_t subset_allreduces = 0;       // exchange steps of the last scanrs_mat_sum_rows_*_sharded (and kin) on this handle (an unsharded one: 0)
    uint64_t sseq_moment_walks = 0;       // the last sseq_params on this handle: walks over the nonzeros for the moments, 1 under one quantum, 2 with a quantum per gene (the class walk first)
    const int *skip_flag = nullptr;       // device flag the dense kernels launched now test first (nonzero: return at once) — set around the queued passes of a device-side orthonormalisation
    uint64_t orth_fallbacks = 0;          // orthonormalisations that ended in the host Gram-Schmidt for rank-deficient panels (solver.cpp)
    uint64_t bk_host_retries = 0;         // svd_bk calls that fell back from the device-side factorizations to the host path (scanrs_mat_get_counter)
    // what the last svd_bk on this handle decided about its reused projection (host-side stores, scanrs_mat_get_counter "bk_*"; a retry
    // on the host path overwrites them): limit_branch 0 = no older column flagged, 1 = the flagged ones fit the repair pass, 2 = bound
    // raised to the largest flagged, 3 = raised to `need`, 4 = bound unchanged and a pass wider than 104 columns
    struct BkDecisions {
        uint64_t q = 0, b = 0, coef_valid = 0, flagged_older = 0, limit_branch = 0, direct_columns = 0, last_direct = 0, full_direct = 0,
                 early_projections = 0;
        double limit = 0.0, cmax_dense = 0.0; // the bound finally used; the largest max|C| among the columns that took the dense route
    } bk;
    // the route of the last sparse product on this handle (host-side stores by launch_spmm_f64, overwritten on every call;
    // scanrs_mat_get_counter "spmm_route" / "spmm_form" / "spmm_chunks", packed as scanrs_amd.h documents; spmm_route.hpp)
    struct SpmmDecision {
        uint64_t family = 0, form = 0, chunks = 0;
    } spmm;
    ~Storage();
    // the copy whose outer dimension is the base matrix's rows (true) or cols (false)
    SparseCopy &copy_with_outer_rows(bool outer_rows);
};
struct Storage::SideBuild {
    std::thread th;
    hipStream_t stream = nullptr;
    // what the helper makes, in this order: [copy of `first` if it does not exist] -> layout of `first` -> [copy of `second`] -> layout
    // of `second`; a waiter needs one copy (or its layout) and waits for that stage only
    const SparseCopy *order[2] = {nullptr, nullptr};
    bool want_layout[2] = {false, false};
    std::mutex mu;
    std::condition_variable cv;
    bool copy_done[2] = {false, false}, layout_done[2] = {false, false}; // by position in `order`
    bool finished = false;
    int code = SCANRS_OK;
    std::string err;
    double ms = 0.0;
};
SCANRS_LOCAL void registry_set_side(Storage &st, Storage::SideBuild *sb); // st.side = sb under the registry's mutex: all_library_streams_idle sees the helper's stream or nothing, never a destroyed one
// THE list of the streams a handle queues work on: f(name, stream) for each one that exists, in this order. The deferred frees
// (one release event per stream), "is the handle idle?" and the destructor's drain all rest on it: a new stream goes here.
template <class F>
void for_each_stream(const Storage &st, F &&f) {
    const std::pair<const char *, hipStream_t> all[] = {{"main", st.stream}, {"aux", st.aux_stream}, {"aux2", st.aux2_stream}, {"overflow", st.ov_stream}, {"helper", st.side ? st.side->stream : nullptr}};
    for (const auto &x : all)
        if (x.second) f(x.first, x.second);
}

// ---- lazy map (sqz::MatrixMap chain) ------------------------------------------------------
enum { OP_INTO = 0, OP_SCALE_AXIS = 1, OP_LN_1P = 2, OP_LOG2_1P = 3, OP_LOG10_1P = 4, OP_SQUARE = 5, OP_BINOM_DEV = 6, OP_BINOM_PEARSON = 7 };
constexpr int MAX_OPS = 8; // SparseCopy::fsig_* are sized to this

uint32_t next_map_op_id(); // runtime.cpp: never reused (1 ..), identifies a link and the arrays it holds
struct MapOp {
    int kind = OP_INTO;
    int axis = 0;
    bool swap = false; // under an odd number of TransposeMap wrappers
    std::shared_ptr<DevBuf<double>> a, b;
    uint32_t id = next_map_op_id(); // copies of a link (views) keep the id: same arrays, same values
};

// what the kernels see (by value)
struct DevOp {
    int kind;
    int a_outer; // index `a` by the outer (1) or inner (0) position of the copy being walked
    int b_outer;
    uint32_t id; // MapOp::id
    const double *a;
    const double *b;
};
struct DevMap {
    int n;
    int _pad;
    DevOp ops[MAX_OPS];
};

inline uint32_t even_up(uint32_t x) { return (x + 1u) & ~1u; }

} // namespace scanrs

// The opaque handle of the C ABI.
struct scanrs_mat {
    std::shared_ptr<scanrs::Storage> st;
    bool transposed = false; // this view is the base matrix transposed
    std::vector<scanrs::MapOp> ops;
    uint32_t off_rank = 0;
    std::shared_ptr<scanrs::DevBuf<double>> off_u; // rows x rank (view coordinates)
    std::shared_ptr<scanrs::DevBuf<double>> off_v; // rank x cols
    double target_umi = 0.0;

    uint64_t rows() const { return transposed ? st->cols : st->rows; }
    uint64_t cols() const { return transposed ? st->rows : st->cols; }
    // is the (view) outer dimension that contracts in V*x sharded?  (see Storage::shard)
    scanrs::DevMap dev_map(bool outer_is_view_row) const;
};

namespace scanrs {

// no link of the handle's map changes a value: it still shows the stored counts
SCANRS_LOCAL inline bool map_is_raw(const scanrs_mat *m) {
    for (const auto &op : m->ops)
        if (op.kind != OP_INTO) return false;
    return true;
}

// CancelProgress::check (snoop/src/lib.rs:37-58): fails with SCANRS_ERR_CANCELLED once the flag is set (sn may be null)
SCANRS_LOCAL inline void snoop_check(const scanrs_snoop *sn) {
    if (sn && sn->cancel && __atomic_load_n(sn->cancel, __ATOMIC_RELAXED)) fail(SCANRS_ERR_CANCELLED, "cancellation error");
}
// CancelProgress::set_progress_check (snoop/src/lib.rs:45-57): the cancel test, then the progress report
SCANRS_LOCAL inline void snoop_poll(const scanrs_snoop *sn, double progress) {
    snoop_check(sn);
    if (sn && sn->progress) sn->progress(sn->ctx, progress);
}

// n values host -> device on stream s (nothing is queued for n == 0; `h` must outlive the copy)
template <typename T>
SCANRS_LOCAL inline void h2d(T *d, const T *h, size_t n, hipStream_t s) {
    if (n) SCANRS_HIP(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s));
}

// ---- kernels.hip: the sparse products and the per-outer-vector reductions ------------------
// out[n_outer x l] = S * X (+ a * w) where S is `cp` seen through `map`.
// off_a: n_outer x rank (row-major) or null; off_w: rank x l (ld = ldw).
void launch_spmm_f64(Storage &st, SparseCopy &cp, const DevMap &map, const double *X, uint32_t ldx, uint32_t l,
                     double *out, uint32_t ldo, const double *off_a, uint32_t rank, const double *off_w, uint32_t ldw);
void launch_spmm_u32(Storage &st, const SparseCopy &cp, const uint32_t *X, uint32_t ldx, uint32_t l, uint32_t *out,
                     uint32_t ldo);
// per-outer-vector reductions. mode 0: sum of raw u32 counts; 1: sum of mapped values; 2: sum and sum of squares.
void launch_row_reduce(Storage &st, SparseCopy &cp, const DevMap &map, int mode, uint32_t *out_u32, double *out_sum,
                       double *out_sumsq);
// cp.bounds: per outer vector the offsets of its nonzeros at multiples of 2^BT_SHIFT = 1024 inner positions (one base tile), built
// on first use on stream `s` (null: the handle's); returns the number of base tiles
constexpr uint32_t BT_SHIFT = 10;
uint32_t ensure_bounds(Storage &st, SparseCopy &cp, hipStream_t s = nullptr);
// fout[p] = the whole chain of `map` at nonzero p of `cp`
void materialize_map_values(Storage &st, SparseCopy &cp, const DevMap &map, double *fout);
// the overflow part of a tile layout through the L2-blocked gather on stream `s` (weights in ov.fvals, no map, no offset)
void launch_gather2d_ov(Storage &st, hipStream_t s, SparseCopy &ov, const double *X, uint32_t ldx, uint32_t l, double *out, uint32_t ldo);
void launch_scale_rows(Storage &st, const double *X, uint32_t ldx, uint64_t rows, uint32_t l, const double *a, double *Xs);
// one empty launch per translation unit that the first create -> normalize -> run_pca reaches (library_warm_up)
void warm_kernels(hipStream_t s);
void warm_panel_ops(hipStream_t s);
void warm_copy_build(hipStream_t s);
void warm_normalize_ops(hipStream_t s);
void warm_dense(hipStream_t s);
void warm_decode(hipStream_t s);
void warm_knn(hipStream_t s);
void warm_knn_metric(hipStream_t s);
void warm_tiles(hipStream_t s);

// ---- tiles.hip (whether a product is a candidate for the tiles at all: spmm_route.hpp) ----------
bool spmm_tiles_auto(Storage &st, SparseCopy &cp, const DevMap &map);
// the structure of the layout (no weights) when the auto path would take it for this copy: built on stream s; false when the copy
// is not eligible or its layout is not worth having (then remembered in cp.tile_rejected_shape)
bool tile_layout_build_auto(Storage &st, SparseCopy &cp, hipStream_t s);
void launch_spmm_tiles(Storage &st, SparseCopy &cp, const DevMap &map, const double *X, uint32_t ldx, uint32_t l, double *out,
                       uint32_t ldo, const double *off_a, uint32_t rank, const double *off_w, uint32_t ldw);
// where the dense tile product of (cp, l) will stage its compact panel copy from — when the caller can fill it while it reads the
// panel anyway (mat_apply: the column sums of the offset term) — or nullptr (another path, a layout about to be rebuilt, odd l)
double *tile_panel_copy_target(Storage &st, SparseCopy &cp, uint32_t l);

// ---- dense.hip: the routes of the dense products, the LDS-tiled and skinny MFMA forms, the factor step --------
// Which kernel a dense product goes to, as pure host functions of the shape (the values are the SCANRS_DENSE_* constants of
// scanrs_amd.h). launch_gram / launch_gemm_nn (panel_ops.hip) call them; the *_route launchers take a route (0: the dispatcher's)
// and refuse a forced kernel whose own preconditions fail (tests: scanrs_debug_dense_*).
enum GramRoute { GRAM_AUTO = 0, GRAM_WAVE = 1, GRAM_VEC = 2, GRAM_TILED = 3 };
enum GemmRoute { GEMM_AUTO = 0, GEMM_WAVE = 1, GEMM_TILED = 2, GEMM_SKINNY_LDS = 3, GEMM_DIRECT = 4 };
struct GemmPlan {
    GemmRoute route;
    uint32_t nt;     // MFMA column tiles per wave: NJ of gemm_nn_kernel, NT of gemm_skinny_direct_kernel (LDS forms: 0)
    uint32_t groups; // column groups (grid.y)
};
inline uint32_t gemm_wave_nj(uint32_t m) { return m <= 16u ? 1u : m <= 32u ? 2u : 4u; } // 16-column MFMA tiles per wave of gemm_nn_kernel
// side: the product is queued on a side stream while dense_side_no_lds is set (register-only forms)
GramRoute gram_route(uint32_t n, uint32_t m, uint64_t rows, uint32_t ldx, uint32_t ldy, bool side, bool skip_flag_set);
GemmPlan gemm_route(bool x_aligned16, uint32_t ldx, uint32_t n, uint32_t m, uint64_t rows, bool side, bool gemm_direct);
// LDS-tiled MFMA versions for big panels
bool gram_tiled_ok(uint32_t n, uint32_t m, uint64_t rows);
bool gemm_tiled_ok(uint32_t n, uint32_t m, uint64_t rows);
void launch_gram_tiled(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *Y, uint32_t ldy, uint32_t m,
                       uint64_t rows, double *C);
bool gemm_direct_ok(const double *X, uint32_t ldx, uint32_t n, uint32_t m, uint64_t rows);
void launch_gemm_direct(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *W, uint32_t ldw, uint32_t m, uint64_t rows,
                        double alpha, double beta, const double *Cin, uint32_t ldc, double *Out, uint32_t ldo);
void launch_gemm_tiled(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *W, uint32_t ldw, uint32_t m,
                       uint64_t rows, double alpha, double beta, const double *Cin, uint32_t ldc, double *Out, uint32_t ldo);
void launch_gemm_skinny_lds(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *W, uint32_t ldw, uint32_t m,
                            uint64_t rows, double alpha, double beta, const double *Cin, uint32_t ldc, double *Out, uint32_t ldo);
// the factor step of CholeskyQR on the device
bool chol_rinv_ok(uint32_t n);
void launch_chol_rinv(Storage &st, const double *G, uint32_t n, uint64_t rows, int pass, bool check_only, int *ctl, double *Rinv, double *info);
void launch_absmax_flag(Storage &st, const double *C, uint32_t count, double limit, int *ctl, double *info);

// ---- panel_ops.hip: dense panel utilities of the solvers ---------------------------------------------
// w[rank x l] (ld ldw) = B^T X, B: n x rank row-major, X: n x l (ld ldx)
void launch_weighted_colsum(Storage &st, const double *B, uint32_t rank, const double *X, uint32_t ldx, uint64_t n,
                            uint32_t l, double *w, uint32_t ldw, double *Xc = nullptr, uint32_t ldc = 0);
// C[n x m] (row-major, ld = m) = X^T Y over `rows` rows (f64 MFMA, slab + ordered reduce)
void launch_gram(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *Y, uint32_t ldy, uint32_t m,
                 uint64_t rows, double *C);
// Out[rows x m] = beta * Cin + alpha * X[rows x n] * W[n x m]   (W device, row-major ld = ldw). Cin may equal Out.
void launch_gemm_nn(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *W, uint32_t ldw, uint32_t m,
                    uint64_t rows, double alpha, double beta, const double *Cin, uint32_t ldc, double *Out, uint32_t ldo);
void launch_gram_route(Storage &st, int route, const double *X, uint32_t ldx, uint32_t n, const double *Y, uint32_t ldy, uint32_t m,
                       uint64_t rows, double *C);
void launch_gemm_route(Storage &st, int route, const double *X, uint32_t ldx, uint32_t n, const double *W, uint32_t ldw, uint32_t m,
                       uint64_t rows, double alpha, double beta, const double *Cin, uint32_t ldc, double *Out, uint32_t ldo);
void launch_col_scale_dev(Storage &st, double *dst, uint32_t ldd, const double *src, uint32_t lds, uint64_t rows, const double *nsq);
void launch_col_axpy_dev(Storage &st, double *y, uint32_t ldy, const double *x, uint32_t ldx, uint64_t rows, const double *nsq);
void launch_col_scale(Storage &st, double *dst, uint32_t ldd, const double *src, uint32_t lds, uint64_t rows, double alpha);
void launch_col_axpy(Storage &st, double *y, uint32_t ldy, const double *x, uint32_t ldx, uint64_t rows, double alpha);
void launch_copy_cols(Storage &st, const double *src, uint32_t lds, double *dst, uint32_t ldd, uint64_t rows, uint32_t l);
void launch_fill_f64(Storage &st, double *p, uint64_t n, double v);
void launch_fill_hash(Storage &st, double *p, uint32_t ld, uint64_t rows, uint64_t row0, uint32_t c0, uint32_t nc, uint64_t seed);
void launch_omega_jump(Storage &st, const uint64_t *d_jpow, int n_pow, const uint64_t s[4], uint64_t d, uint64_t total, double *out,
                       uint32_t ld, uint64_t seq_cols, bool transpose);
void launch_transpose(Storage &st, const double *src, uint64_t rows, uint64_t cols, double *dst, uint32_t ldd);
void launch_permute_cols(Storage &st, const double *src, uint32_t lds, double *dst, uint32_t ldd, uint64_t rows,
                         const uint32_t *d_idx, uint32_t n_idx, bool scatter);

// ---- normalize_ops.hip: the small kernels of normalize ------------------------------------------------
// out_sum[i] (and out_sumsq[i]) over the outer vectors of cp, per INNER position i. false: not eligible (nothing was launched).
bool launch_col_moments(Storage &st, SparseCopy &cp, const DevMap &map, int mode, double *out_sum, double *out_sumsq);
void launch_finish_moments(Storage &st, const double *sum, const double *sumsq, uint64_t n, double m, int given_scale,
                           const double *scale_in, double *mean_over_scale_neg, double *inv_scale, double *scale_out);
void launch_u32_to_scale(Storage &st, const uint32_t *counts, uint64_t n, double target, double *out);
void launch_hist12(Storage &st, const uint32_t *v, uint64_t n, uint32_t shift, uint32_t digit_mask, uint32_t prefix_mask,
                   uint32_t prefix, unsigned long long *hist);
void launch_sum_f64(Storage &st, const double *x, uint64_t n, double *out);
void launch_densify(Storage &st, const SparseCopy &cp, const DevMap &map, bool outer_is_view_row, uint64_t cols_v,
                    double *out);
void launch_binom_uv(Storage &st, int kind, const double *n, uint64_t ncols, const double *rowsum, uint64_t nrows,
                     double total, double *pi, double *u, double *v);

// ---- copy_build.hip: construction of a SparseCopy (with SparseCopy::build_items) -----------------------
void validate_copy(Storage &st, SparseCopy &cp, uint64_t *zeros, uint64_t *bad);
// build `dst` = transpose of `src` (stable: inner vectors keep ascending outer order)
void build_transposed_copy(Storage &st, const SparseCopy &src, SparseCopy &dst, hipStream_t stream = nullptr);
// drop stored zeros, compact (device). Returns new nnz.
void compact_nonzeros(Storage &st, SparseCopy &cp);
void sort_outer_vectors(Storage &st, SparseCopy &cp);

// ---- host_linalg.cpp --------------------------------------------------------------------------
// Upper Cholesky G = R^T R of an n x n SPD matrix (row-major, in place: upper triangle = R). false if not SPD.
bool chol_upper(double *g, int n);
// in place inverse of an upper-triangular matrix
void inv_upper(double *r, int n);
// symmetric eigen-decomposition: on return w[0..n) descending, z row-major with z[i*n + j] = component i of vector j.
bool sym_eig(const double *a, int n, double *w, double *z);
// k leading eigenpairs only: w[0..k) descending, z row-major n x k
bool sym_eig_topk(const double *a, int n, int k, double *w, double *z);

// ---- solver.cpp ------------------------------------------------------------------------------------
int pca_bk(scanrs_mat *m, uint32_t k, double k_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
           const scanrs_snoop *snoop, double *u, double *s, double *v);
int pca_rand(scanrs_mat *m, uint32_t k, double l_multiplier, uint32_t n_iter, uint64_t seed, const double *omega, double *u,
             double *s, double *v);
int pca_irlba(scanrs_mat *m, uint32_t nu, double tol, uint32_t max_iter, const double *v0, const scanrs_snoop *snoop,
              double *u, double *s, double *v, uint32_t *mprod);
void omega_fill(uint64_t seed, uint64_t count, double *out);
void jump_tables_prefetch(); // starts the background computation of the start panel generator's jump tables (once per process)

// operator-level helpers shared by capi.cpp and solver.cpp
// out[rows_v x l] = V * X  (transpose: out[cols_v x l] = V^T * X), offsets and shard reduction included.
void mat_apply(scanrs_mat *m, bool transpose, const double *dX, uint32_t ldx, uint32_t l, double *dOut, uint32_t ldo);
void prepare_second_orientation(scanrs_mat *m, bool transpose_second, bool solver_follows = false);
// knn.hip
void knn_host(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k, bool skip_same_index,
              uint32_t *out);
// the same with both point sets already in device memory (row-major, leading dimensions in elements); `out` is a host array
void knn_device(const double *d_queries, uint32_t ld_q, uint64_t n_q, const double *d_points, uint32_t ld_p, uint64_t n_p, uint32_t d,
                uint32_t k, bool skip_same_index, uint32_t *out, double *sq_dist = nullptr); // sq_dist: host, n_q x k squared distances (+inf in padded slots), or nullptr
// The collective search of a sharded handle, on the handle's stream: d_pts holds the rank's own rows [begin, begin + n_local)
// of the n global ones; out / sq_dist are host arrays over the rank's rows and hold GLOBAL indices. Counts st.knn_blocks / knn_allreduces.
void knn_sharded(Storage &st, const double *d_pts, uint32_t ld, uint64_t begin, uint64_t n_local, uint64_t n, uint32_t d, uint32_t k,
                 uint32_t *out, double *sq_dist);
// the merge rule of that search on host arrays (knn_merge.hpp; scanrs_host_knn_merge)
void knn_host_merge(uint32_t k, const double *da, const uint32_t *ia, const double *db, const uint32_t *ib, double *dout, uint32_t *iout);
// for tests (scanrs_debug_knn_*): what the last knn_device of the process did, one entry per filter round (nothing when it did not go
// through the filter); the filter's constants; one filter pass on host arrays
void knn_last_stats(bool &filtered, uint64_t &first_stride, std::vector<uint64_t> &strides, std::vector<uint64_t> &points,
                    std::vector<uint64_t> &cand_sum, std::vector<uint32_t> &cand_max, std::vector<uint32_t> &overflowed);
void knn_filter_params(double &gamma, uint32_t &cap, uint32_t &dmax, uint32_t &k_max, uint64_t &nq_min, double &coord_min, double &coord_max);
void knn_filter_debug(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, const double *tau, uint64_t stride,
                      uint32_t *cnt, uint32_t *cand);
// decode.hip
uint64_t decode_adaptive_vectors(const scanrs_adaptive_vec *vecs, uint64_t n_vecs, uint64_t vec_len, DevBuf<uint64_t> &indptr,
                                 DevBuf<uint32_t> &indices, DevBuf<uint32_t> &values, uint64_t *uploaded_bytes = nullptr);
// encode.hip: the encoders (the inverse direction). One entry per outer vector: its encoding, stored entries and fallback entries;
// byte_off / word_off (n_outer + 1 entries) place its pieces in the two device arenas: `data` (padded to 8 bytes), then index_bytes
// (S*) in d_bytes; fallback indexes, fallback values, then block_starts (S*) in d_words.
struct EncodedVec {      // written by the plan kernel, read by the emit kernels and, as it is, by the host
    uint32_t kind, n;    // encoding, stored entries
    uint32_t n_fb, _pad; // fallback entries
    uint64_t fb_base;    // the plan's own bookkeeping: entries before the vector's first that reach its marker
};
void encode_adaptive_vectors(Storage &st, const SparseCopy &cp, int force_kind, std::vector<EncodedVec> &vecs, std::vector<uint64_t> &byte_off,
                             std::vector<uint64_t> &word_off, DevBuf<uint64_t> &d_bytes, DevBuf<uint32_t> &d_words);
// reshard.hip / reshard_host.cpp: the inner-sharding constructors of multi.cpp. A slab: a run of the caller's outer vectors.
void launch_reshard_count(hipStream_t s, const SparseCopy &slab, uint32_t *d_counts); // d_counts[j] += stored entries at inner position j (zeroed by the caller)
// d_start ((world + 1) x slab.n_outer): where destination d's run of every vector begins; d_moved[d] += the runs' lengths (zeroed by the caller)
void launch_reshard_split(hipStream_t s, const SparseCopy &slab, const uint64_t *d_bounds, uint32_t world, uint64_t *d_start,
                          unsigned long long *d_moved);
// the destination's side, reading a source's slab in place: rows d / d + 1 of its start table, the kept entries per run, then the copy
void launch_reshard_len(hipStream_t s, const uint64_t *d_from, const uint64_t *d_to, const uint32_t *d_values, uint64_t n_vec, bool has_zeros,
                        unsigned long long *d_len);
void launch_reshard_pull(hipStream_t s, const uint64_t *d_from, const uint64_t *d_to, const uint32_t *d_indices, const uint32_t *d_values,
                         uint64_t n_vec, uint32_t rebase, const uint64_t *d_out_ptr, uint32_t *d_out_idx, uint32_t *d_out_val);
void reshard_check_frame(uint64_t n_outer, uint64_t n_inner, const uint64_t *indptr, const uint32_t *indices, bool values_given);
void reshard_host_plan(const uint64_t *indptr, const uint32_t *indices, uint64_t n_outer, uint64_t n_inner, uint32_t world, uint64_t *slab_bounds,
                       uint64_t *bounds, uint64_t *moved);
// regather.hip / regather_host.cpp: scanrs_multi_gather_outer and scanrs_multi_rebalance (multi.cpp). The sources of a
// pull as the kernels take them, by value: shard s holds the outer vectors [bounds[s], bounds[s + 1]) of the source matrix in its own
// arrays (nnz[s] entries; on the destination's device or a peer's).
constexpr uint32_t REGATHER_TILE = 2048;   // output elements a workgroup of the pull owns
constexpr uint32_t REGATHER_MAX_SHARDS = 16;
struct RegatherSources {
    uint32_t n = 0, _pad = 0;
    uint64_t bounds[REGATHER_MAX_SHARDS + 1] = {};
    uint64_t nnz[REGATHER_MAX_SHARDS] = {};
    const uint64_t *indptr[REGATHER_MAX_SHARDS] = {};
    const uint32_t *indices[REGATHER_MAX_SHARDS] = {};
    const uint32_t *values[REGATHER_MAX_SHARDS] = {};
};
// d_len (n_vec + 1 entries): the length of source vector d_list[j] for every output vector j (+ the scan's spare entry);
// d_place[j]: its source shard and where it begins in that shard's arrays
void launch_regather_len(hipStream_t s, const RegatherSources &src, const uint32_t *d_list, uint64_t n_vec, unsigned long long *d_len, uint64_t *d_place);
// the nnz entries of the destination (d_indptr: its n_vec + 1 offsets), every one read at its place in a source's arrays
void launch_regather_pull(hipStream_t s, const RegatherSources &src, const uint64_t *d_indptr, const uint64_t *d_place, uint64_t n_vec, uint64_t nnz,
                          uint32_t *d_out_idx, uint32_t *d_out_val);
// the plan on host arrays (scanrs_host_plan_gather; the device path runs the same function on the indptr it assembled from the shards):
// out_indptr (n_idx + 1): the selected matrix's; bounds (n_dst + 1): scanrs_plan_shards over it; moved (n_src x n_dst, source-major).
// Any output may be null. Refusals: a null list, shard counts outside 1 .. 16, source bounds that do not tile the outer extent
// (SCANRS_ERR_ARGUMENT); an index beyond the outer extent (SCANRS_ERR_INVALID).
void regather_host_plan(const uint64_t *indptr, uint64_t n_outer, const uint64_t *src_bounds, uint32_t n_src, const uint64_t *idx, uint64_t n_idx,
                        uint32_t n_dst, uint64_t *out_indptr, uint64_t *bounds, uint64_t *moved);
void regather_check_list(const uint64_t *idx, uint64_t n_idx, uint64_t n_outer);
// export_multi.hip / encode_host.cpp: scanrs_multi_to_adaptive (multi.cpp). The sources of the INNER pull are the shards'
// TRANSPOSED copies: source s holds all n_inner vectors over its own outer range [bounds[s], bounds[s + 1]), indices local.
// A destination's slab: the n_vec inner positions from g0 on, over all outer positions.
// d_len (n_vec + 1 entries): the length of every slab vector over all sources (+ the scan's spare entry)
void launch_export_len(hipStream_t s, const RegatherSources &src, uint64_t g0, uint64_t n_vec, unsigned long long *d_len);
// d_start ((src.n + 1) x n_vec): where source s's piece of every slab vector begins in the slab (d_indptr: the slab's n_vec + 1 offsets)
void launch_export_start(hipStream_t s, const RegatherSources &src, uint64_t g0, uint64_t n_vec, const uint64_t *d_indptr, uint64_t *d_start);
// the nnz entries of the slab, every one read at its place in a source's arrays, its index raised by the source's outer_begin
void launch_export_pull(hipStream_t s, const RegatherSources &src, uint64_t g0, const uint64_t *d_indptr, const uint64_t *d_start, uint64_t n_vec,
                        uint64_t nnz, uint64_t outer_global, uint32_t *d_out_idx, uint32_t *d_out_val);
// the plan on host arrays (scanrs_host_plan_export; the device path runs the same function on the counts it took from the shards'
// transposed indptr arrays): counts is n_src x n_inner, source-major. out_indptr (n_inner + 1): the whole matrix's inner-major indptr;
// slab_bounds (n_dst + 1): scanrs_plan_shards over it; moved (n_src x n_dst, source-major). Any output may be null. Refusals: a null
// table with entries, shard counts outside 1 .. 16 (SCANRS_ERR_ARGUMENT).
void export_host_plan(const uint64_t *counts, uint32_t n_src, uint64_t n_inner, uint32_t n_dst, uint64_t *out_indptr, uint64_t *slab_bounds,
                      uint64_t *moved);
// The export object as scanrs_multi_to_adaptive fills it (encode_host.cpp): a table of n_vecs entries and n_parts pairs of host arenas.
// adaptive_export_encode runs the encoders over `cp` on st's stream and the current device, brings the two arenas down into part
// `part` and fills the table entries [first_vec, first_vec + cp.n_outer); calls on different parts may run on different threads.
// *arena_bytes: the bytes of the two arenas that crossed the host link. adaptive_export_finish sums the parts' accounting and records
// what the multi call did (scanrs_adaptive_export_multi_info).
scanrs_adaptive_export *adaptive_export_new(uint64_t n_vecs, uint32_t n_parts);
void adaptive_export_encode(scanrs_adaptive_export *e, uint32_t part, Storage &st, const SparseCopy &cp, int force_kind, uint64_t first_vec,
                            uint64_t *arena_bytes);
void adaptive_export_finish(scanrs_adaptive_export *e, const std::vector<uint64_t> &slab_bounds, const std::vector<uint64_t> &moved,
                            const std::vector<uint64_t> &arena_bytes);
void adaptive_check_export_args(const void *handle, int major, int force_kind, scanrs_adaptive_export **out);
// capi.cpp: a registered Storage with its main stream on the current device (what every handle starts from)
SCANRS_LOCAL std::shared_ptr<Storage> new_storage(uint64_t rows, uint64_t cols, int storage);
// comm.cpp
struct LocalGroup;
void comm_allreduce(Storage &st, scanrs_comm *c, void *d, uint64_t count, int dtype); // dtype 0 = f64, 1 = u64; on st.stream
void comm_abort(scanrs_comm *c);
std::shared_ptr<LocalGroup> local_group_make(uint32_t world);
void local_group_reset(LocalGroup &g);
scanrs_comm *comm_make_local(const std::shared_ptr<LocalGroup> &g, uint32_t rank);
void allreduce_f64(Storage &st, double *d, uint64_t count);
void allreduce_u64(Storage &st, unsigned long long *d, uint64_t count);
// is the view-row dimension the sharded one?
bool rows_sharded(const scanrs_mat *m);
bool cols_sharded(const scanrs_mat *m);
// the cells of a handle as its collective calls see them: [begin, begin + n_local) of `global` (an unsharded handle: all of them)
struct CellRange {
    uint64_t begin, n_local, global;
};
inline CellRange cell_range(const Storage &st, uint64_t cells_local) {
    if (!st.shard.active()) return CellRange{0, cells_local, cells_local};
    return CellRange{st.shard.outer_begin, cells_local, st.shard.outer_global};
}

// ---- sseq.hip / sseq_host.cpp: sSeq differential expression (diff-exp/src/diff_exp.rs, dist.rs) --------------------------------
constexpr uint32_t SSEQ_CHUNK_THREADS = 256, SSEQ_TERMS_PER_THREAD = 8, SSEQ_CHUNK = SSEQ_CHUNK_THREADS * SSEQ_TERMS_PER_THREAD;
constexpr uint32_t SSEQ_MAX_GROUPS = 8192; // one wave's LDS row of u64 group sums fills 64 KB
struct SseqExactTest {       // one exact test: terms k = 0 .. n, chunks chunk0 .. (next test's chunk0)
    uint64_t n, xa;
    double sar, sbr, add_total; // sf_a / φ, sf_b / φ, the constant of log_prob_all
    uint64_t chunk0, out;       // first chunk; index of the p-value in the output
};
struct SseqAsymTest {
    uint64_t xa, xb;
    double sf_a, sf_b, mu, phi;
    uint64_t out;
};
struct SseqRatioTest {       // one exact test of the Ratio backend (sseq_ratio.inc): ceil(anchor / SSEQ_CHUNK) chunks below the anchor, then
    uint64_t n, xa, anchor;  // ceil((n - anchor) / SSEQ_CHUNK) above it; anchor: the first k whose step is below 1, else n (dist.rs:178-184)
    double sar, sbr;
    uint64_t chunk0, out;
};
constexpr double SSEQ_RATIO_FALLBACK = -1.0; // written in place of a p-value: the test has to go through the LogSpace kernels
uint32_t sseq_max_count(Storage &st, const SparseCopy &cp);
void launch_sseq_cell_totals(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t n_cells, unsigned long long *d_tot);
// sums: genes x n_groups; with d_mom also Σ x/sf and Σ (x/sf)² over the labelled cells as 128-bit fixed point (genes x 4 u64), under
// scale1 / scale2, or with d_cls under every gene's own scales (fixed128.hpp: its class and log2m, 2^log2m >= the number of labelled cells)
void launch_sseq_group_pass(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t n_genes, const int16_t *d_labels, uint32_t n_groups,
                            unsigned long long *d_sums, const double *d_sf, double scale1, double scale2, unsigned long long *d_mom,
                            uint32_t *d_bad, const uint32_t *d_cls = nullptr, int log2m = 0);
// per gene the class of its largest finite x/sf_c over the labelled cells of this copy (0: none)
void launch_sseq_term_class(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t n_genes, const int16_t *d_labels, const double *d_sf,
                            uint32_t *d_cls);
// sharded handles: the two 128-bit sums and the bad flag of every gene as u64 limbs (genes x SSEQ_LIMB_STRIDE) for the u64 all-reduce, and back
constexpr uint32_t SSEQ_LIMB_STRIDE = 9;
void launch_sseq_mom_split(Storage &st, const unsigned long long *d_mom, const uint32_t *d_bad, uint64_t n_genes, unsigned long long *d_limbs);
void launch_sseq_mom_join(Storage &st, const unsigned long long *d_limbs, uint64_t n_genes, unsigned long long *d_mom, uint32_t *d_bad);
void launch_sseq_exact(hipStream_t s, const SseqExactTest *d_tests, uint32_t n_tests, uint64_t n_chunks, double *d_obs, double4 *d_part,
                       double *d_p);
void launch_sseq_asymptotic(hipStream_t s, const SseqAsymTest *d_tests, uint32_t n_tests, double *d_p);
void launch_sseq_ratio(hipStream_t s, const SseqRatioTest *d_tests, uint32_t n_tests, uint64_t n_chunks, double *d_obs, double *d_scale,
                       double2 *d_part, double *d_p);
// host side (sseq_host.cpp); `cp` is the resident copy, gene_major when its outer vectors are the genes (the view's rows)
void sseq_params(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, double zeta_quintile,
                 const uint64_t *cell_indices, uint64_t n_sel, const double *umi_counts, double *size_factors, double *gene_means,
                 double *gene_variances, uint8_t *use_genes, double *gene_moment_phi, double *zeta_hat, double *delta, double *gene_phi);
void sseq_params_from_moments(const double *mean_g, const double *var_g, uint64_t n, double sum_size_factors, double n_cells, double n_genes,
                              double zeta_quintile, uint8_t *use_genes, double *gene_moment_phi, double *zeta_hat, double *delta,
                              double *gene_phi);
void sseq_group_sums(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, const int16_t *labels,
                     uint32_t n_groups, uint64_t *sums, uint64_t *cells_per_group);
void sseq_de_matrix(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, const int16_t *labels,
                    uint32_t n_groups, int mode, const double *size_factors, const double *gene_means, const double *gene_phi,
                    const uint8_t *use_genes, uint64_t big_count, const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p,
                    double *p_adj, double *log2fc, double *mean_in, double *mean_out, int backend = SCANRS_NB_EXACT_LOGSPACE);
// the tests, BH, log2 fold change and normalized means from per-gene sums (genes x n_tests, row-major)
void sseq_de_sums(hipStream_t s, uint64_t genes, uint32_t n_tests, const uint64_t *sums_a, const uint64_t *sums_b, const double *sf_a,
                  const double *sf_b, const double *gene_means, const double *gene_phi, const uint8_t *use_genes, uint64_t big_count,
                  const scanrs_snoop *snoop, double *p, double *p_adj, double *log2fc, double *mean_in, double *mean_out,
                  int backend = SCANRS_NB_EXACT_LOGSPACE);
// the same with the parameters read per (gene, test): gene_means / gene_phi / use_genes at [g * stride_g + j * stride_j]. (1, 0) is
// sseq_de_sums (one set of parameters for every test), (n_tests, 1) a genes x n_tests array (scanrs_sseq_de_pairs)
void sseq_de_sums_strided(hipStream_t s, uint64_t genes, uint32_t n_tests, const uint64_t *sums_a, const uint64_t *sums_b, const double *sf_a,
                          const double *sf_b, const double *gene_means, const double *gene_phi, const uint8_t *use_genes, uint64_t stride_g,
                          uint64_t stride_j, uint64_t big_count, const scanrs_snoop *snoop, double *p, double *p_adj, double *log2fc,
                          double *mean_in, double *mean_out, int backend, Storage *shard = nullptr);
// the copy DE walks: the gene-major one when it is resident, else the cell-major one (shared with merge_clusters). A sharded handle is
// served when its cells (the view's columns) are the sharded dimension; sseq_refuse_sharded is for the entry points that do not serve one.
SCANRS_LOCAL SparseCopy &sseq_resident_copy(scanrs_mat *m, bool *gene_major);
SCANRS_LOCAL void sseq_refuse_sharded(const scanrs_mat *m, const char *what);
double sseq_host_exact_test(uint64_t xa, uint64_t xb, double sf_a, double sf_b, double mu, double phi);
double sseq_host_exact_test_ratio(uint64_t xa, uint64_t xb, double sf_a, double sf_b, double mu, double phi);
uint64_t sseq_ratio_anchor(uint64_t n, double sar, double sbr);
void sseq_host_bh(const double *p, uint64_t n, double *out);

// ---- sseq_pairs.hip / sseq_pairs_host.cpp: batched pairwise DE with per-pair parameters (diff_exp.rs:361-376, merge_clusters.rs) ----
struct SseqPairHeader {  // one pair (a, b) of groups: what its tests need besides the per-gene accumulators
    double m_s;          // interpolated median total of the union (percentile_of_sorted(.., 50), stat.rs:140-162)
    double n_s, sum_sf;  // cells of the union; Σ 1/sf_c over its cells with a total = m_S Σ 1/u_c
    double sf_a, sf_b;   // Σ_A u / m_S, Σ_B u / m_S
    uint64_t n_a, n_b;
    uint32_t a, b, literal, pad; // literal: m_S == 0, the pair takes compute_sseq_params + mode 1 DE
};
// d_tot[perm[i]] -> d_sorted[i], each group's segment [off[g], off[g + 1]) sorted ascending; d_stats (n_groups x 3 u64): Σ u, Σ 1/u (lo, hi)
void launch_pairs_group_stats(hipStream_t s, const unsigned long long *d_tot, const uint32_t *d_perm, const uint32_t *d_off, uint32_t n_groups,
                              uint64_t n_labelled, double scale, unsigned long long *d_gathered, unsigned long long *d_sorted,
                              unsigned long long *d_stats, DevBuf<char> &sort_tmp);
void launch_pairs_headers(hipStream_t s, const unsigned long long *d_sorted, const uint32_t *d_off, const unsigned long long *d_stats,
                          const uint32_t *d_pair_a, const uint32_t *d_pair_b, uint32_t n_pairs, double scale, SseqPairHeader *d_hdr);
// per (gene, pair), genes x n_pairs row-major: the moments of the union, use_genes, the method-of-moments dispersion, both sides' sums
void launch_pairs_moments(hipStream_t s, const unsigned long long *d_acc, const SseqPairHeader *d_hdr, uint64_t genes, uint32_t n_pairs,
                          double scale, double *d_mean, double *d_var, uint8_t *d_use, double *d_phi_mm, unsigned long long *d_sums_a,
                          unsigned long long *d_sums_b);
// per pair: zeta_hat, delta (d_zd: n_pairs x 2) and gene_phi (diff_exp.rs:409-441)
void launch_pairs_shrink(hipStream_t s, const double *d_phi_mm, const uint8_t *d_use, uint64_t genes, uint32_t n_pairs, double pct, double *d_zd,
                         double *d_phi);
// sharded handles: a tile of `ne` (group, gene) entries of the grouped accumulators (5 u64 each; the tile starts at an even
// entry) as SSEQ_ACC_PLANES planes of u64 that add up without overflow over the ranks (planes x ne rounded up to even), and back with the
// carries propagated. sseq_reduce_group_acc all-reduces the whole table in tiles of SSEQ_ACC_TILE entries through a scratch of
// SSEQ_ACC_PLANES x SSEQ_ACC_TILE u64 (56 MiB, whatever the table's size) and returns the exchange steps it made (counted in
// de_shard_allreduces); on an unsharded handle it does nothing.
constexpr uint32_t SSEQ_ACC_PLANES = 7;
constexpr uint64_t SSEQ_ACC_TILE = 1ull << 20;
void launch_pairs_acc_split(hipStream_t s, const unsigned long long *d_acc_tile, uint64_t ne, unsigned long long *d_planes);
void launch_pairs_acc_join(hipStream_t s, const unsigned long long *d_planes, uint64_t ne, unsigned long long *d_acc_tile);
uint64_t sseq_reduce_group_acc(Storage &st, unsigned long long *d_acc, uint64_t n_entries);
// the batched pairwise DE (sseq_pairs_host.cpp). collective: a sharded handle is served (cells = the rank's own), labels span the whole matrix
void sseq_de_pairs(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, const int16_t *labels, uint32_t n_groups,
                   const uint32_t *pair_a, const uint32_t *pair_b, uint32_t n_pairs, double zeta_quintile, uint64_t big_count, int backend,
                   const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc, double *mean_in,
                   double *mean_out, scanrs_sseq_pair_params *params, bool collective = false);

// ---- cluster.hip / cluster_host.cpp: merge_clusters (scan-rs/src/merge_clusters.rs, linkage.rs) ---------------------------------
constexpr uint32_t MERGE_MAX_CLUSTERS = 8192;
constexpr uint32_t MERGE_TILE_CLUSTERS = 1536; // clusters of one gene-major tile: a wave's LDS row of 5 u64 each fills 60 KB
// exact medians of every (cluster, column): d_perm lists the cells cluster by cluster, d_off (n_clusters + 1) their segments;
// d_keys holds n x cols_per_tile u64; d_nan_cell gets the smallest cell index holding a NaN (or all ones); d_out n_clusters x d
void launch_medoids(hipStream_t s, const double *d_scores, uint64_t n, uint32_t ld, uint32_t d, const uint32_t *d_perm, const uint64_t *d_off,
                    uint32_t n_clusters, unsigned long long *d_keys, uint32_t cols_per_tile, unsigned long long *d_nan_cell, double *d_out);
// the fused pass of merge_clusters: d_out (n_clusters x genes x 5 u64) = Σ x, Σ x/u (lo, hi), Σ (x/u)² (lo, hi) per (cluster, gene);
// returns the passes over the nonzeros it made (gene-major: one per tile of MERGE_TILE_CLUSTERS clusters)
uint32_t launch_merge_pass(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t n_genes, const int16_t *d_labels, uint32_t n_clusters,
                           const unsigned long long *d_tot, double scale1, double scale2, unsigned long long *d_out);
uint32_t merge_tile_clusters(uint32_t n_clusters);
// distributed exact medians: the cells of a (cluster, column) segment lie on several ranks, so a radix round is a local
// histogram per (pair, wanted rank), one u64 all-reduce of the table and a replicated pick. Pair p = jj * n_clusters + cluster of a column
// tile; d_state holds 4 u64 per pair (prefix and remaining rank of ⌊(len-1)/2⌋ and ⌊len/2⌋); d_hist 512 u64 per pair of a tile of at most
// MEDOID_HIST_PAIRS pairs (16 MiB, whatever the number of clusters and columns). d_len: the clusters' GLOBAL cell counts.
constexpr uint32_t MEDOID_HIST_PAIRS = 4096;
void launch_medoid_keys(hipStream_t s, const double *d_scores, uint64_t n, uint32_t ld, uint32_t j0, uint32_t jt, const uint32_t *d_perm,
                        unsigned long long *d_keys, unsigned long long *d_nan_cell);
void launch_medoid_dist_init(hipStream_t s, const uint64_t *d_len, uint32_t n_clusters, uint32_t jt, unsigned long long *d_state);
void launch_medoid_dist_hist(hipStream_t s, const unsigned long long *d_keys, uint64_t n, const uint64_t *d_off, uint32_t n_clusters, uint32_t p0,
                             uint32_t np, int shift, const unsigned long long *d_state, unsigned long long *d_hist);
void launch_medoid_dist_pick(hipStream_t s, const unsigned long long *d_hist, uint32_t p0, uint32_t np, int shift, unsigned long long *d_state);
void launch_medoid_dist_finish(hipStream_t s, const unsigned long long *d_state, const uint64_t *d_len, uint32_t n_clusters, uint32_t j0, uint32_t jt,
                               double *d_out, uint32_t ldo);
// host side (cluster_host.cpp)
void cluster_pdist(const double *x, uint64_t m, uint32_t d, double *out);
void cluster_linkage_complete(const double *x, uint64_t m, uint32_t d, double *z);
void cluster_relabel_by_size(const int16_t *labels, uint64_t n, int16_t *out);
void cluster_check_labels(const int16_t *labels, uint64_t n, uint32_t k);
uint32_t cluster_count_labels(const int16_t *labels, uint64_t n); // K of a valid labelling (checked)
void cluster_medoids(hipStream_t s, const double *d_scores, uint64_t n, uint32_t ld, uint32_t d, const int16_t *labels, uint32_t k, double *centers);
void merge_clusters_run(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, const double *d_scores, uint32_t ld,
                        uint32_t d, const int16_t *labels, int16_t *labels_out, const scanrs_snoop *snoop, scanrs_merge_trace *trace,
                        bool collective = false);
// the m - 1 merges [a, b, distance, .] in discovery order -> rows by (distance, discovery row), named through the union-find
void cluster_sort_relabel(const double *z, uint64_t m, double *z_out);

// ---- hclust.hip / hclust_host.cpp: hierarchical clustering (hclust/src/lib.rs) -----------------------------------------------------
// d_obs (n x d compact) from x (rows or columns of it are the observations); *d_bad = the first element of x that is not finite, or all ones
void launch_hclust_pack(hipStream_t s, const double *d_x, uint64_t n, uint32_t d, uint64_t ld, int by_cols, double *d_obs, unsigned long long *d_bad);
// d_dist: the full symmetric n x n matrix of (squared) Euclidean distances; *d_bad_pair (may be null) = the first pair i * n + j, i < j,
// whose distance is not finite, or all ones
void launch_hclust_pdist(hipStream_t s, const double *d_obs, uint64_t n, uint32_t d, int squared, double *d_dist, unsigned long long *d_bad_pair);
// one step of the nearest-neighbour chain, two launches: d_ctr = {chain length, merges, steps, error}, d_rec 5 u32
void launch_hclust_step(hipStream_t s, double *d_dist, uint32_t n, int method, uint32_t *d_chain, uint32_t *d_size, unsigned long long *d_ctr,
                        uint32_t *d_rec, uint32_t *d_ma, uint32_t *d_mb, double *d_mh, uint32_t *d_msize);

// ---- select.hip / select_host.cpp: select_rows, select_cols, partition_on_thresholds (sqz/src/mat.rs:730-888, 1004-1071) ---------
void launch_sel_outer_sums(hipStream_t s, const SparseCopy &cp, const uint8_t *excl_outer, const uint8_t *excl_inner, unsigned long long *out);
void launch_sel_inner_sums(hipStream_t s, const SparseCopy &cp, const uint8_t *pick, uint8_t want, bool subtract, const uint8_t *excl_inner,
                           unsigned long long *sums);
void launch_sel_mark(hipStream_t s, const unsigned long long *sums, uint64_t n, double threshold, uint8_t *excl, uint8_t *newly, uint32_t *flag);
void select_scan_offsets(hipStream_t s, unsigned long long *d, uint64_t n); // in place: n lengths (+ one spare entry) -> n + 1 offsets
void launch_part_count(hipStream_t s, const SparseCopy &cp, const int32_t *pos_a, const int32_t *pos_b, const int32_t *remap, bool cols_inner,
                       unsigned long long *len_a, unsigned long long *len_b);
void launch_part_fill(hipStream_t s, const SparseCopy &cp, const int32_t *pos_a, const int32_t *pos_b, const int32_t *remap, bool cols_inner,
                      const uint64_t *ip_a, uint32_t *idx_a, uint32_t *val_a, const uint64_t *ip_b, uint32_t *idx_b, uint32_t *val_b);
void launch_gather_len(hipStream_t s, const SparseCopy &cp, const uint32_t *d_idx, uint64_t n_idx, unsigned long long *len);
void launch_gather_copy(hipStream_t s, const SparseCopy &cp, const uint32_t *d_idx, uint64_t n_idx, const uint64_t *ip_out, uint32_t *idx_out,
                        uint32_t *val_out);
void launch_expand_count(hipStream_t s, const SparseCopy &cp, const uint32_t *inv_ptr, unsigned long long *len);
void launch_expand_fill(hipStream_t s, const SparseCopy &cp, const uint32_t *inv_ptr, const uint32_t *inv_pos, const uint64_t *ip_out,
                        uint32_t *idx_out, uint32_t *val_out);
// host side (select_host.cpp). `out` receives indptr / indices / values, the dimensions and nnz of the new matrix in cp's orientation
// (no work items: the handle that adopts it builds them). idx: n_idx valid positions of the named axis, any order, repeats allowed.
void select_outer(Storage &st, const SparseCopy &cp, const uint64_t *idx, uint64_t n_idx, SparseCopy &out);
void select_inner(Storage &st, const SparseCopy &cp, const uint64_t *idx, uint64_t n_idx, SparseCopy &out);
// thr_outer / thr_inner: nullable thresholds of the two axes of cp; cols_inner: the view's columns are cp's inner positions (their
// step comes first in a round). excl_outer / excl_inner: the final masks (host). filtered / residual may be null (not built).
// Returns the number of rounds. sh (a sharded handle): cp is the rank's shard; excl_outer, filtered and residual stay
// local, excl_inner is replicated, sh receives what the call learned about the whole outer dimension, and the exchange steps are added
// to st.partition_allreduces.
struct PartitionShard {
    std::vector<uint8_t> excl_outer_all; // the outer mask of the whole matrix (outer_global entries), the same on every rank
};
uint64_t partition_on_thresholds(Storage &st, const SparseCopy &cp, const double *thr_outer, const double *thr_inner, bool cols_inner,
                                 std::vector<uint8_t> &excl_outer, std::vector<uint8_t> &excl_inner, SparseCopy *filtered, SparseCopy *residual,
                                 PartitionShard *sh = nullptr);
// the outer-axis selection of a sharded handle: idx holds positions of the WHOLE outer dimension, non-decreasing; this rank takes the
// run that falls into [outer_begin, outer_begin + cp.n_outer). *out_begin: the entries below the rank's range (the result's outer_begin)
void select_outer_sharded(Storage &st, const SparseCopy &cp, const uint64_t *idx, uint64_t n_idx, SparseCopy &out, uint64_t *out_begin);

// ---- subset.hip / subset_host.cpp: sum_rows, sum_cols, sum_rows_dual, mean_rows, mean_var_rows (sqz/src/mat.rs:279-282, 333-374, 414-583) ----
// d_list: n distinct positions (u32) on the device. mode 0: u64 sums of the raw counts, 1: f64 sums of the mapped values, 2: f64 sum and
// sum of squares (one list). Results: d_out[k * stride + position], k = the list (or 0 = sum, 1 = sum of squares).
void launch_subset_code(Storage &st, const uint32_t *d_list, uint64_t n, uint8_t bit, uint8_t *d_code); // d_code[list[i]] |= bit
void launch_subset_pos(Storage &st, const uint32_t *d_list, uint64_t n, uint32_t *d_pos);               // d_pos[list[i]] = i
// masked walk over cp's work items; d_slab: 2 values per slab row of cp (cp.n_slab rows), d_code: one byte per inner position
void launch_subset_reduce(Storage &st, const SparseCopy &cp, const DevMap &map, int mode, int n_sets, const uint8_t *d_code, void *d_out,
                          uint64_t stride, void *d_slab);
void launch_subset_finish(Storage &st, const SparseCopy &cp, int mode, int n_k, const void *d_slab, void *d_out, uint64_t stride);
// d_out[d_pos[inner]] += count over all of cp (d_out zeroed by the caller; d_pos: 0xFFFFFFFF where not listed)
void launch_subset_inner_scatter(Storage &st, const SparseCopy &cp, const uint32_t *d_pos, unsigned long long *d_out);
// the listed outer vectors of cp: d_out[i] = sum of vector d_list[i] (mode 0 or 1) / d_out[inner] += count (d_out zeroed by the caller)
void launch_subset_listed(Storage &st, const SparseCopy &cp, const DevMap &map, int mode, const uint32_t *d_list, uint64_t n, void *d_out);
void launch_subset_listed_scatter(Storage &st, const SparseCopy &cp, const uint32_t *d_list, uint64_t n, unsigned long long *d_out);
// The fixed-point forms of the two f64 walks, for sums that cross the shards: every term is rounded once to the quantum
// 1 / scale (fixed128.hpp, signed) and summed in 128-bit integers. d_fx: 4 u64 per result (lo, hi of the first sum, lo, hi of the
// second: list 2 of a dual call under scale1, or the sum of squares of mode 2 under scale2), d_bad: one flag per result (a term was not
// finite, or did not fit the quantum). d_slab: 5 u64 per slab row of cp. Both arrays are written for every result.
void launch_subset_reduce_fx(Storage &st, const SparseCopy &cp, const DevMap &map, int mode, int n_sets, const uint8_t *d_code, double scale1,
                             double scale2, unsigned long long *d_fx, uint32_t *d_bad, unsigned long long *d_slab);
void launch_subset_listed_fx(Storage &st, const SparseCopy &cp, const DevMap &map, const uint32_t *d_list, uint64_t n, double scale1,
                             unsigned long long *d_fx, uint32_t *d_bad);
// the pre-pass of the quantum: *d_max (zeroed by the caller) = the bit pattern of the largest finite |mapped value| over the listed
// nonzeros: the masked walk (positions with a nonzero byte in d_code) or the listed vectors
void launch_subset_reduce_max(Storage &st, const SparseCopy &cp, const DevMap &map, const uint8_t *d_code, unsigned long long *d_max);
void launch_subset_listed_max(Storage &st, const SparseCopy &cp, const DevMap &map, const uint32_t *d_list, uint64_t n, unsigned long long *d_max);
// n_sums (1 or 2) 128-bit sums and the flag of every result as 32-bit limbs held in u64 (n x (4 n_sums + 1)) around the u64 all-reduce,
// and back (the kin of launch_sseq_mom_split / _join)
void launch_subset_fx_split(Storage &st, const unsigned long long *d_fx, const uint32_t *d_bad, uint64_t n, int n_sums, unsigned long long *d_limbs);
void launch_subset_fx_join(Storage &st, const unsigned long long *d_limbs, uint64_t n, int n_sums, unsigned long long *d_fx, uint32_t *d_bad);

} // namespace scanrs
