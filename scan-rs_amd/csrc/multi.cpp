// multi.cpp — the single-process multi-GPU form of the boundary (`mat_create(..., n_gpus)`).
// Cell Ranger is one process (tools/src/bin/cmd.rs:61-70): it hands over the whole matrix once and calls normalize
// and run_pca once. Here the outer vectors are range-partitioned by nonzeros over `n_shards` devices, every shard is an
// ordinary scanrs_mat handle on its own device driven by its own host thread for the duration of a call, and the
// exchange steps go through the library's single-process group (comm.cpp). Several shards may share one device
// (`devices` repeats an id): that is how a 1-GPU box exercises the whole path. A matrix that arrives feature-major (the reference's
// own orientation) is sharded over its INNER dimension by the constructors further down (scanrs_multi_create_inner); an
// existing scanrs_multi is cut anew, reordered or moved to other devices by scanrs_multi_gather_outer / _rebalance (§7n), and the whole
// matrix leaves as AdaptiveVec encodings, in either orientation, through scanrs_multi_to_adaptive at the end (§7p).
#include <functional>
#include <thread>

#include "common.hpp"

struct scanrs_multi {
    uint64_t rows = 0, cols = 0;
    int storage = SCANRS_CSR;
    std::vector<int> devices;
    std::vector<uint64_t> bounds; // n_shards + 1, in outer vectors
    std::vector<scanrs_mat *> shards;
    std::vector<scanrs_comm *> comms;
    std::shared_ptr<scanrs::LocalGroup> group;
    // what an inner-sharding constructor did (scanrs_multi_create_info); null on every other scanrs_multi
    struct InnerInfo {
        std::vector<uint64_t> slab_bounds, moved, uploaded;
    };
    std::shared_ptr<InnerInfo> inner;
    // what scanrs_multi_gather_outer / _rebalance did (scanrs_multi_gather_info); null on every other scanrs_multi
    struct GatherInfo {
        uint32_t n_src = 0;
        std::vector<uint64_t> bounds, moved, host_bytes;
    };
    std::shared_ptr<GatherInfo> gather;
};

using namespace scanrs;

namespace {

struct ShardStatus {
    int code = SCANRS_OK;
    std::string msg;
};

// run f(i) for every shard on its own thread with its device current; first failure wins (cancellation over the
// secondary "another shard failed")
template <typename F>
int fan_out(scanrs_multi *mm, F &&f) {
    const size_t n = mm->shards.size();
    std::vector<ShardStatus> st(n);
    std::vector<std::thread> th;
    // a failed or cancelled earlier operation aborted its own barriers only: the handle stays usable (no shard thread runs here)
    if (mm->group) local_group_reset(*mm->group);
    for (size_t i = 0; i < n; i++) {
        th.emplace_back([&, i] {
            if (hipSetDevice(mm->devices[i]) != hipSuccess) {
                st[i].code = SCANRS_ERR_DEVICE;
                st[i].msg = "hipSetDevice failed";
            } else {
                st[i].code = f(i);
                if (st[i].code != SCANRS_OK) st[i].msg = scanrs_last_error();
            }
            if (st[i].code != SCANRS_OK && i < mm->comms.size()) comm_abort(mm->comms[i]); // wake the others out of their barriers
        });
    }
    for (auto &t : th) t.join();
    int first = SCANRS_OK;
    size_t who = 0;
    for (size_t i = 0; i < n; i++) {
        if (st[i].code == SCANRS_OK) continue;
        const bool secondary = st[i].msg.find("another shard") != std::string::npos;
        if (first == SCANRS_OK || (!secondary && st[who].msg.find("another shard") != std::string::npos)) {
            first = st[i].code;
            who = i;
        }
    }
    if (first != SCANRS_OK) set_error("shard %zu: %s", who, st[who].msg.c_str());
    return first;
}

int bad_argument(const char *msg) {
    set_error("%s", msg);
    return SCANRS_ERR_ARGUMENT;
}

// ---- the constructor frame: what everything that makes a scanrs_multi shares ------------------------------------
// 1 <= n_shards <= 16 in the words of the entry point (`msg` may print the count with %u)
void check_shard_count(uint32_t n_shards, const char *msg) {
    if (n_shards == 0 || n_shards > REGATHER_MAX_SHARDS) fail(SCANRS_ERR_ARGUMENT, msg, n_shards);
}

// the checks of scanrs_multi_create, which every inner-sharding constructor inherits (a missing triplet is refused in the words of a bad count)
void check_frame(bool have_triplet, uint32_t n_shards, int storage, scanrs_multi **out) {
    if (!out) fail(SCANRS_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    check_shard_count(have_triplet ? n_shards : 0, "1 <= n_shards <= 16 and a triplet are required");
    if (storage != SCANRS_CSR && storage != SCANRS_CSC) fail(SCANRS_ERR_ARGUMENT, "storage must be 0 (CSR) or 1 (CSC)");
}

// `from` maps the memory of `to` (the one-shot all-reduce reads peers' partial sums in place, a destination of gather_outer a source's arrays)
void enable_peer(int from, int to) {
    if (from == to) return;
    int can = 0;
    SCANRS_HIP(hipDeviceCanAccessPeer(&can, from, to));
    if (!can) fail(SCANRS_ERR_DEVICE, "devices %d and %d cannot map each other's memory", from, to);
    SCANRS_HIP(hipSetDevice(from));
    const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) SCANRS_HIP(e);
    (void)hipGetLastError();
}

// the devices of a new scanrs_multi (`devices` null: 0 .. n_shards-1; ids may repeat), peer access between every pair of distinct ones,
// the group and one communicator per shard
void bind_devices(scanrs_multi *mm, uint32_t n_shards, const int *devices) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) fail(SCANRS_ERR_DEVICE, "no gfx950 (MI355X) device is usable from this process");
    for (uint32_t i = 0; i < n_shards; i++) {
        const int d = devices ? devices[i] : (int)i;
        if (d < 0 || d >= n_dev) fail(SCANRS_ERR_ARGUMENT, "device %d of shard %u does not exist (%d visible)", d, i, n_dev);
        mm->devices.push_back(d);
    }
    for (uint32_t i = 0; i < n_shards; i++)
        for (uint32_t j = 0; j < n_shards; j++) enable_peer(mm->devices[i], mm->devices[j]);
    mm->group = local_group_make(n_shards);
    mm->shards.assign(n_shards, nullptr);
    for (uint32_t i = 0; i < n_shards; i++) mm->comms.push_back(comm_make_local(mm->group, i));
}

// shard i's empty handle of the given local shape, made on the current device and published: from here on scanrs_multi_free takes the
// storage down
scanrs_mat *make_shard(scanrs_multi *mm, size_t i, uint64_t rows, uint64_t cols) {
    auto stp = new_storage(rows, cols, mm->storage);
    auto *h = new scanrs_mat();
    h->st = stp;
    mm->shards[i] = h;
    return h;
}

// Finishes shard d over a validated copy as scanrs_mat_create finishes a handle: the largest stored count (validate_copy's), the work
// items (of an empty copy only with `items_always`), then() for what the constructor still builds from the copy, the flush on the
// idle stream, and the shard's communicator and range out of `outer_global`.
template <typename F>
void finish_shard(scanrs_multi *mm, size_t d, SparseCopy &cp, bool items_always, uint64_t outer_global, F &&then) {
    scanrs_mat *h = mm->shards[d];
    Storage &st = *h->st;
    cp.max_value = cp.nnz ? std::max(sseq_max_count(st, cp), 1u) : 0u;
    if (cp.nnz || items_always) cp.build_items(st.stream);
    then();
    device_free_flush();
    if (const int rc = scanrs_mat_set_shard_comm(h, mm->comms[d], (uint32_t)d, (uint32_t)mm->shards.size(), mm->bounds[d], outer_global)) throw Failure{rc};
}

extern "C" { // (free_shards and shard_snoop have C names in the library's symbol table, which this file leaves as it found it)

void free_shards(scanrs_multi *mm, std::vector<scanrs_mat *> &made) {
    for (size_t i = 0; i < made.size(); i++) {
        if (!made[i]) continue;
        (void)hipSetDevice(mm->devices[i]);
        scanrs_mat_free(made[i]);
        made[i] = nullptr;
    }
}

// the snoop of shard i: every shard polls the cancel flag at the same points; only shard 0 reports progress
const scanrs_snoop *shard_snoop(const scanrs_snoop *snoop, size_t i, scanrs_snoop &sn) {
    if (!snoop) return nullptr;
    sn = *snoop;
    if (i != 0) sn.progress = nullptr;
    return &sn;
}

} // extern "C"

// the failure path of everything that makes handles: free_all() takes down what was made, and freeing handles must not replace the
// message of the failure
template <typename F>
int failed(int rc, F &&free_all) {
    const std::string msg = scanrs_last_error();
    free_all();
    set_error("%s", msg.c_str());
    return rc;
}

// ---- the collective frame: one call of the handle on every shard at once ---------------------------------------------------
// Every shard gets the same global arguments and computes the same complete outputs; shard 0 writes the caller's arrays, the others
// write into scratch of the call. Every shard polls the cancel flag at the same points; only shard 0 reports progress.
struct ShardView { // the handle a shard's call runs on: the shard itself, or its transposed view for the length of the call
    scanrs_mat *h = nullptr;
    bool owned = false;
    int open(scanrs_multi *mm, size_t i, int transposed) {
        if (!transposed) {
            h = mm->shards[i];
            return SCANRS_OK;
        }
        owned = true;
        return scanrs_mat_t(mm->shards[i], &h);
    }
    ~ShardView() {
        if (owned && h) scanrs_mat_free(h);
    }
};

// the outputs of one shard's call: the caller's array on shard 0, a zeroed array of the call's own on every other shard
class ShardOutputs {
    struct Block {
        std::unique_ptr<void, void (*)(void *)> mem;
    };
    const bool first;
    std::vector<Block> owned; // each a separate allocation, released with the call

  public:
    explicit ShardOutputs(size_t shard) : first(shard == 0) {}
    // an output of n elements (one more is allocated: never an empty array)
    template <typename T>
    T *out(T *callers, size_t n) {
        if (first) return callers;
        owned.push_back(Block{{new T[n + 1](), [](void *p) { delete[] static_cast<T *>(p); }}});
        return static_cast<T *>(owned.back().mem.get());
    }
    // an output the caller may leave out, which only shard 0 fills
    template <typename T>
    T *optional(T *callers) const {
        return first ? callers : nullptr;
    }
};

// body(i, handle, snoop, outputs) on every shard, on its transposed view where `transposed`, with the snoop narrowed for the shard
template <typename F>
int collective(scanrs_multi *mm, int transposed, const scanrs_snoop *snoop, F &&body) {
    return fan_out(mm, [&](size_t i) {
        ShardView v;
        if (const int rc = v.open(mm, i, transposed)) return rc;
        scanrs_snoop sn;
        ShardOutputs o(i);
        return (int)body(i, v.h, shard_snoop(snoop, i, sn), o);
    });
}

} // namespace

extern "C" {

int scanrs_multi_create(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices,
                        const uint32_t *values, uint32_t n_shards, const int *devices, scanrs_multi **out) {
    return guard([&] {
        check_frame(indptr != nullptr, n_shards, storage, out);
        auto mm = std::make_unique<scanrs_multi>();
        mm->rows = rows;
        mm->cols = cols;
        mm->storage = storage;
        bind_devices(mm.get(), n_shards, devices);
        const uint64_t n_outer = storage == SCANRS_CSR ? rows : cols;
        mm->bounds.resize(n_shards + 1);
        if (scanrs_plan_shards(indptr, n_outer, n_shards, mm->bounds.data()) != SCANRS_OK) throw Failure{SCANRS_ERR_ARGUMENT};
        scanrs_multi *raw = mm.get();
        const int rc = fan_out(raw, [&](size_t i) {
            const uint64_t lo = raw->bounds[i], hi = raw->bounds[i + 1];
            std::vector<uint64_t> ip(hi - lo + 1);
            for (uint64_t o = lo; o <= hi; o++) ip[o - lo] = indptr[o] - indptr[lo];
            const uint64_t r = storage == SCANRS_CSR ? hi - lo : rows, c = storage == SCANRS_CSR ? cols : hi - lo;
            int rc2 = scanrs_mat_create(r, c, storage, ip.data(), indices + indptr[lo], values + indptr[lo], &raw->shards[i]);
            if (rc2 != SCANRS_OK) return rc2;
            return scanrs_mat_set_shard_comm(raw->shards[i], raw->comms[i], (uint32_t)i, (uint32_t)raw->shards.size(), lo, n_outer);
        });
        if (rc != SCANRS_OK) throw Failure{failed(rc, [&] { scanrs_multi_free(mm.release()); })};
        *out = mm.release();
    });
}

// ---- the inner-sharding constructors (mat.rs:68-124, hdf5-io/src/matrix.rs:119-192, mtx.rs:10-51, cmd.rs:61-70) -----------
// The matrix arrives in the reference's orientation (genes x cells CSR: one vector per gene) and the shards of the result own ranges of
// its INNER dimension (the cells), stored the other way round. Nothing is transposed on the host and every nonzero is uploaded once:
//   1  the outer vectors are dealt in n_shards slabs by nonzeros; shard s uploads slab s, validates it (validate_copy, before any
//      kernel indexes by an inner index) and counts its stored entries per inner position;
//   2  the counts are summed on the host, scanned, and scanrs_plan_shards gives `bounds`: exactly what scanrs_multi_create plans for
//      the transposed triplet; every shard then finds, per vector and destination, the run of entries that belongs to it
//      (launch_reshard_split: indices ascend inside a vector, so a run lies between two lower bounds);
//   3  every destination reads its runs out of every source's slab in slab order (in place: the same device's memory, or a peer's
//      through the peer mapping), the index rebased and stored zeros dropped: the CSR of ALL outer vectors x its own inner range;
//   4  the slabs are released, and build_transposed_copy (stable: inner indices ascend) makes the shard's stored orientation.
// The phases are separate fan_outs: the join of the shard threads is the barrier between them, and a failing shard ends its phase.
} // extern "C"

namespace {

struct InnerShard { // what shard s holds on its device while the constructor runs
    SparseCopy slab; // its slab as uploaded: slab.n_outer vectors over all n_inner positions, stored zeros still in
    uint64_t zeros = 0;
    DevBuf<uint32_t> counts;
    std::vector<uint32_t> h_counts;
    DevBuf<uint64_t> start; // (n_shards + 1) x slab.n_outer (launch_reshard_split)
    SparseCopy piece;       // all outer vectors x the shard's own inner range
    void drop_slab() {
        slab = SparseCopy();
        counts.release();
        start.release();
    }
};

// wall clock of a phase on a shard's thread, added to Storage::reshard_us[which] (every phase ends on an idle stream)
struct PhaseClock {
    uint64_t &slot;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit PhaseClock(uint64_t &s) : slot(s) {}
    ~PhaseClock() { slot += (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
};

// slab [lo, hi) of shard s onto the current device (the arrays of `slab`, nnz; n_outer / n_inner are set); `uploaded`: bytes that crossed the host link
using SlabLoader = std::function<void(size_t s, uint64_t lo, uint64_t hi, Storage &st, SparseCopy &slab, uint64_t &uploaded)>;

int create_inner(uint64_t rows, uint64_t cols, int storage, const std::vector<uint64_t> &slab_bounds, const SlabLoader &load, uint32_t n_shards,
                 const int *devices, scanrs_multi **out) {
    const uint64_t n_outer = storage == SCANRS_CSR ? rows : cols, n_inner = storage == SCANRS_CSR ? cols : rows;
    const int out_storage = storage == SCANRS_CSR ? SCANRS_CSC : SCANRS_CSR; // the same rows x cols, stored the other way round
    auto mm = std::make_unique<scanrs_multi>();
    mm->rows = rows;
    mm->cols = cols;
    mm->storage = out_storage;
    bind_devices(mm.get(), n_shards, devices);
    mm->bounds.assign(n_shards + 1, 0);
    mm->inner = std::make_shared<scanrs_multi::InnerInfo>();
    scanrs_multi::InnerInfo &info = *mm->inner;
    info.slab_bounds = slab_bounds;
    info.moved.assign((size_t)n_shards * n_shards, 0);
    info.uploaded.assign(n_shards, 0);
    std::vector<InnerShard> work(n_shards);
    scanrs_multi *raw = mm.get();
    jump_tables_prefetch(); // as scanrs_mat_create does: the seeded start panel's tables, off the first PCA's path

    // 1: upload, validate, count
    int rc = fan_out(raw, [&](size_t s) {
        return guard([&] {
            need_device();
            Storage &st = *make_shard(raw, s, 0, 0)->st; // (its shape is known once `bounds` is)
            CurrentHandle cur(&st);
            InnerShard &w = work[s];
            w.slab.n_outer = slab_bounds[s + 1] - slab_bounds[s];
            w.slab.n_inner = n_inner;
            {
                PhaseClock clock(st.reshard_us[0]);
                load(s, slab_bounds[s], slab_bounds[s + 1], st, w.slab, info.uploaded[s]);
            }
            PhaseClock clock(st.reshard_us[1]);
            uint64_t bad = 0;
            validate_copy(st, w.slab, &w.zeros, &bad);
            if (bad) fail(SCANRS_ERR_ARGUMENT, "indices must be in range and strictly ascending within each outer vector (%llu violations)", (unsigned long long)bad);
            w.counts.alloc(std::max<uint64_t>(1, n_inner));
            SCANRS_HIP(hipMemsetAsync(w.counts.p, 0, std::max<uint64_t>(1, n_inner) * 4, st.stream));
            launch_reshard_count(st.stream, w.slab, w.counts.p);
            w.h_counts.assign(n_inner, 0);
            if (n_inner) SCANRS_D2H(w.h_counts.data(), w.counts.p, n_inner * 4, st.stream);
            SCANRS_SYNC(st.stream);
            w.counts.release();
        });
    });

    // the plan: the transposed indptr from the summed counts, cut as scanrs_multi_create would cut it
    if (rc == SCANRS_OK)
        rc = guard([&] {
            std::vector<uint64_t> tip(n_inner + 1, 0);
            for (uint32_t s = 0; s < n_shards; s++) {
                const std::vector<uint32_t> &c = work[s].h_counts;
                for (uint64_t j = 0; j < n_inner; j++) tip[j + 1] += c[j];
                std::vector<uint32_t>().swap(work[s].h_counts);
            }
            for (uint64_t j = 0; j < n_inner; j++) tip[j + 1] += tip[j];
            if (scanrs_plan_shards(tip.data(), n_inner, n_shards, raw->bounds.data()) != SCANRS_OK) throw Failure{SCANRS_ERR_ARGUMENT};
        });

    // 2: the runs of every (vector, destination)
    if (rc == SCANRS_OK)
        rc = fan_out(raw, [&](size_t s) {
            return guard([&] {
                Storage &st = *raw->shards[s]->st;
                CurrentHandle cur(&st);
                InnerShard &w = work[s];
                PhaseClock clock(st.reshard_us[2]);
                const uint64_t nv = w.slab.n_outer;
                DevBuf<uint64_t> d_bounds(n_shards + 1), d_moved(n_shards);
                SCANRS_HIP(hipMemcpyAsync(d_bounds.p, raw->bounds.data(), (n_shards + 1) * 8, hipMemcpyHostToDevice, st.stream));
                SCANRS_HIP(hipMemsetAsync(d_moved.p, 0, n_shards * 8, st.stream));
                w.start.alloc(std::max<uint64_t>(1, (uint64_t)(n_shards + 1) * nv));
                launch_reshard_split(st.stream, w.slab, d_bounds.p, n_shards, w.start.p, reinterpret_cast<unsigned long long *>(d_moved.p));
                SCANRS_D2H(&info.moved[s * n_shards], d_moved.p, n_shards * 8, st.stream);
                SCANRS_SYNC(st.stream); // the table is complete before any destination reads it (the join below publishes it)
            });
        });

    // 3: every destination gathers its runs from every slab, in slab order
    if (rc == SCANRS_OK)
        rc = fan_out(raw, [&](size_t d) {
            return guard([&] {
                Storage &st = *raw->shards[d]->st;
                CurrentHandle cur(&st);
                SparseCopy &pc = work[d].piece;
                PhaseClock clock(st.reshard_us[3]);
                const uint64_t lo = raw->bounds[d], hi = raw->bounds[d + 1];
                pc.n_outer = n_outer;
                pc.n_inner = hi - lo;
                pc.indptr.alloc(n_outer + 1); // lengths, then (scanned in place) offsets
                SCANRS_HIP(hipMemsetAsync(pc.indptr.p, 0, (n_outer + 1) * 8, st.stream));
                for (uint32_t s = 0; s < n_shards; s++) {
                    const InnerShard &src = work[s];
                    const uint64_t nv = src.slab.n_outer;
                    launch_reshard_len(st.stream, src.start.p + d * nv, src.start.p + (d + 1) * nv, src.slab.values.p, nv, src.zeros != 0,
                                       reinterpret_cast<unsigned long long *>(pc.indptr.p + slab_bounds[s]));
                }
                select_scan_offsets(st.stream, reinterpret_cast<unsigned long long *>(pc.indptr.p), n_outer);
                pc.nnz = SCANRS_D2H_VALUE(pc.indptr.p + n_outer, st.stream);
                pc.indices.alloc(std::max<uint64_t>(1, pc.nnz));
                pc.values.alloc(std::max<uint64_t>(1, pc.nnz));
                for (uint32_t s = 0; s < n_shards && pc.nnz; s++) {
                    const InnerShard &src = work[s];
                    const uint64_t nv = src.slab.n_outer;
                    launch_reshard_pull(st.stream, src.start.p + d * nv, src.start.p + (d + 1) * nv, src.slab.indices.p, src.slab.values.p, nv, (uint32_t)lo,
                                        pc.indptr.p + slab_bounds[s], pc.indices.p, pc.values.p);
                }
                SCANRS_SYNC(st.stream); // nobody's slab is released before every destination has read it (the join below)
            });
        });

    // 4: the slab goes, then the shard's stored orientation is built and bound
    if (rc == SCANRS_OK)
        rc = fan_out(raw, [&](size_t d) {
            return guard([&] {
                Storage &st = *raw->shards[d]->st;
                CurrentHandle cur(&st);
                InnerShard &w = work[d];
                PhaseClock clock(st.reshard_us[4]);
                w.drop_slab();
                device_free_flush(); // the stream is idle here
                // (the largest count sizes the sort keys of the transposition)
                finish_shard(raw, d, w.piece, false, n_inner, [&] {
                    build_transposed_copy(st, w.piece, st.primary);
                    w.piece = SparseCopy();
                    const uint64_t n_loc = raw->bounds[d + 1] - raw->bounds[d];
                    st.rows = out_storage == SCANRS_CSR ? n_loc : rows;
                    st.cols = out_storage == SCANRS_CSR ? cols : n_loc;
                });
            });
        });

    // whatever is left of the temporaries goes back under the handle that made it (a failure; nothing after a success)
    const auto drop_work = [&] {
        for (uint32_t s = 0; s < n_shards; s++) {
            (void)hipSetDevice(raw->devices[s]);
            CurrentHandle cur(raw->shards[s] && raw->shards[s]->st ? raw->shards[s]->st.get() : nullptr, true);
            work[s].drop_slab();
            work[s].piece = SparseCopy();
        }
    };
    if (rc != SCANRS_OK)
        return failed(rc, [&] {
            drop_work();
            scanrs_multi_free(mm.release());
        });
    drop_work();
    *out = mm.release();
    return SCANRS_OK;
}

} // namespace

extern "C" {

int scanrs_multi_create_inner(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices, const uint32_t *values,
                              uint32_t n_shards, const int *devices, scanrs_multi **out) {
    return guard([&] {
        check_frame(true, n_shards, storage, out);
        const uint64_t n_outer = storage == SCANRS_CSR ? rows : cols, n_inner = storage == SCANRS_CSR ? cols : rows;
        reshard_check_frame(n_outer, n_inner, indptr, indices, values != nullptr);
        std::vector<uint64_t> sb(n_shards + 1);
        if (scanrs_plan_shards(indptr, n_outer, n_shards, sb.data()) != SCANRS_OK) throw Failure{SCANRS_ERR_ARGUMENT};
        const SlabLoader load = [&](size_t, uint64_t lo, uint64_t hi, Storage &st, SparseCopy &slab, uint64_t &uploaded) {
            const uint64_t nv = hi - lo, z = indptr[hi] - indptr[lo];
            std::vector<uint64_t> ip(nv + 1);
            for (uint64_t o = lo; o <= hi; o++) ip[o - lo] = indptr[o] - indptr[lo];
            slab.nnz = z;
            slab.indptr.alloc(nv + 1);
            slab.indices.alloc(std::max<uint64_t>(1, z));
            slab.values.alloc(std::max<uint64_t>(1, z));
            SCANRS_HIP(hipMemcpyAsync(slab.indptr.p, ip.data(), (nv + 1) * 8, hipMemcpyHostToDevice, st.stream));
            if (z) {
                SCANRS_HIP(hipMemcpyAsync(slab.indices.p, indices + indptr[lo], z * 4, hipMemcpyHostToDevice, st.stream));
                SCANRS_HIP(hipMemcpyAsync(slab.values.p, values + indptr[lo], z * 4, hipMemcpyHostToDevice, st.stream));
            }
            SCANRS_SYNC(st.stream); // `ip` and the caller's (possibly pageable) arrays are done with
            uploaded = 8 * z + 8 * (nv + 1);
        };
        if (const int rc = create_inner(rows, cols, storage, sb, load, n_shards, devices, out)) throw Failure{rc};
    });
}

int scanrs_multi_create_adaptive_inner(uint64_t rows, uint64_t cols, int storage, const scanrs_adaptive_vec *vecs, uint64_t n_vecs, uint32_t n_shards,
                                       const int *devices, scanrs_multi **out) {
    return guard([&] {
        check_frame(true, n_shards, storage, out);
        const uint64_t n_outer = storage == SCANRS_CSR ? rows : cols, n_inner = storage == SCANRS_CSR ? cols : rows;
        if (n_outer > 0xFFFFFFFFull || n_inner > 0xFFFFFFFFull) fail(SCANRS_ERR_SHAPE, "dimensions must fit in u32 (AdaptiveVec limit)");
        if (n_vecs != n_outer) fail(SCANRS_ERR_SHAPE, "one AdaptiveVec per outer vector is required");
        if (n_vecs > 0 && !vecs) fail(SCANRS_ERR_ARGUMENT, "null vector table");
        // the slabs are cut by the entries the vectors store (n_units: every field of a dense encoding, the entries of a sparse one);
        // the nonzeros themselves are known only once a slab has been expanded on its device
        std::vector<uint64_t> units(n_vecs + 1, 0), sb(n_shards + 1);
        for (uint64_t i = 0; i < n_vecs; i++) units[i + 1] = units[i] + vecs[i].n_units;
        if (scanrs_plan_shards(units.data(), n_vecs, n_shards, sb.data()) != SCANRS_OK) throw Failure{SCANRS_ERR_ARGUMENT};
        const SlabLoader load = [&](size_t, uint64_t lo, uint64_t hi, Storage &, SparseCopy &slab, uint64_t &uploaded) {
            slab.nnz = decode_adaptive_vectors(vecs + lo, hi - lo, n_inner, slab.indptr, slab.indices, slab.values, &uploaded);
            ::scanrs::wait_device(__PRETTY_FUNCTION__, __FILE__, __LINE__); // the decoder works on the null stream
        };
        if (const int rc = create_inner(rows, cols, storage, sb, load, n_shards, devices, out)) throw Failure{rc};
    });
}

int scanrs_multi_create_from_file(const char *path, const char *retain_feature_like, int64_t shrink_row, uint32_t n_shards, const int *devices,
                                  scanrs_multi **out, scanrs_h5_matrix **meta) {
    if (out) *out = nullptr;
    if (meta) *meta = nullptr;
    if (!path || !out) return bad_argument("null argument");
    const size_t n = strlen(path);
    const bool is_h5 = n > 3 && strcmp(path + n - 3, ".h5") == 0;
    scanrs_h5_matrix *h = nullptr;
    int rc = is_h5 ? scanrs_h5_read_adaptive_csr_matrix(path, retain_feature_like, shrink_row, &h) : scanrs_mtx_read(path, &h);
    if (rc != SCANRS_OK) return rc;
    uint64_t rows = 0, cols = 0, nnz = 0;
    int storage = 0;
    const uint64_t *ip = nullptr;
    const uint32_t *ix = nullptr, *vv = nullptr;
    (void)scanrs_h5_matrix_shape(h, &rows, &cols, &nnz, &storage);
    (void)scanrs_h5_matrix_arrays(h, &ip, &ix, &vv);
    rc = scanrs_multi_create_inner(rows, cols, storage, ip, ix, vv, n_shards, devices, out);
    if (rc == SCANRS_OK && meta)
        *meta = h;
    else
        scanrs_h5_matrix_free(h);
    return rc;
}

int scanrs_multi_create_info(const scanrs_multi *mm, uint64_t *slab_bounds, uint64_t *moved, uint64_t *uploaded_bytes) {
    if (!mm) return bad_argument("null handle");
    if (!mm->inner) return bad_argument("create_info: this scanrs_multi was not made by an inner-sharding constructor (scanrs_multi_create_inner and kin)");
    const scanrs_multi::InnerInfo &info = *mm->inner;
    if (slab_bounds) std::copy(info.slab_bounds.begin(), info.slab_bounds.end(), slab_bounds);
    if (moved) std::copy(info.moved.begin(), info.moved.end(), moved);
    if (uploaded_bytes) std::copy(info.uploaded.begin(), info.uploaded.end(), uploaded_bytes);
    return SCANRS_OK;
}

void scanrs_multi_free(scanrs_multi *mm) {
    if (!mm) return;
    for (size_t i = 0; i < mm->shards.size(); i++) {
        (void)hipSetDevice(mm->devices[i]);
        scanrs_mat_free(mm->shards[i]);
    }
    for (auto *c : mm->comms) scanrs_comm_free(c);
    delete mm;
}

int scanrs_multi_n_shards(const scanrs_multi *mm, uint32_t *n) {
    if (!mm || !n) return SCANRS_ERR_ARGUMENT;
    *n = (uint32_t)mm->shards.size();
    return SCANRS_OK;
}

int scanrs_multi_shard(scanrs_multi *mm, uint32_t i, scanrs_mat **shard, int *device, uint64_t *outer_begin, uint64_t *outer_end) {
    if (!mm || i >= mm->shards.size()) return SCANRS_ERR_ARGUMENT;
    if (shard) *shard = mm->shards[i];
    if (device) *device = mm->devices[i];
    if (outer_begin) *outer_begin = mm->bounds[i];
    if (outer_end) *outer_end = mm->bounds[i + 1];
    return SCANRS_OK;
}

int scanrs_multi_comm_info(scanrs_multi *mm, uint32_t i, uint32_t *nranks, uint32_t *rank, uint64_t *n_allreduce, uint64_t *allreduce_bytes) {
    if (!mm || i >= mm->comms.size()) return SCANRS_ERR_ARGUMENT;
    return scanrs_comm_info(mm->comms[i], nranks, rank, n_allreduce, allreduce_bytes);
}

int scanrs_multi_normalize(scanrs_multi *mm, int normalization, const uint32_t *size_factors) {
    if (!mm) return SCANRS_ERR_ARGUMENT;
    return fan_out(mm, [&](size_t i) {
        // size factors are per column: the local slice when the columns are the sharded dimension
        const uint32_t *sf = size_factors;
        if (sf && mm->storage == SCANRS_CSC) sf += mm->bounds[i];
        return scanrs_normalize(mm->shards[i], normalization, sf);
    });
}

// u: rows x k, s: k, v: cols x k (row-major, caller-allocated; u and/or v may be null). The factor on the sharded side
// is assembled from the shards' rows, the replicated one is taken from shard 0.
// call(i, handle, snoop, outputs, u_i, s_i, v_i) under the collective frame; u_i / v_i are null where the shard has nothing to write.
namespace {
extern "C++" template <typename F>
int multi_pca(scanrs_multi *mm, uint32_t k, const scanrs_snoop *snoop, double *u, double *s, double *v, F &&call) {
    if (!mm || !s) return SCANRS_ERR_ARGUMENT;
    const bool cols_sharded = mm->storage == SCANRS_CSC;
    return collective(mm, 0, snoop, [&](size_t i, scanrs_mat *h, const scanrs_snoop *sn, ShardOutputs &o) {
        double *ui = nullptr, *vi = nullptr; // (the replicated factor of shards > 0 is not downloaded)
        if (cols_sharded) {
            ui = (i == 0) ? u : nullptr;
            vi = v ? v + mm->bounds[i] * k : nullptr;
        } else {
            ui = u ? u + mm->bounds[i] * k : nullptr;
            vi = (i == 0) ? v : nullptr;
        }
        return call(i, h, sn, o, ui, o.out(s, k), vi);
    });
}
} // namespace

int scanrs_multi_pca_bk(scanrs_multi *mm, uint32_t k, double k_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
                        const scanrs_snoop *snoop, double *u, double *s, double *v) {
    return multi_pca(mm, k, snoop, u, s, v, [&](size_t, scanrs_mat *h, const scanrs_snoop *sn, ShardOutputs &, double *ui, double *si, double *vi) {
        return scanrs_pca_bk(h, k, k_multiplier, n_iter, seed, omega, sn, ui, si, vi);
    });
}

int scanrs_multi_pca_rand(scanrs_multi *mm, uint32_t k, double l_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
                          double *u, double *s, double *v) {
    return multi_pca(mm, k, nullptr, u, s, v, [&](size_t, scanrs_mat *h, const scanrs_snoop *, ShardOutputs &, double *ui, double *si, double *vi) {
        return scanrs_pca_rand(h, k, l_multiplier, n_iter, seed, omega, ui, si, vi);
    });
}

// Irlba on the un-centred handle (irlba.rs:59-215; LowRankOffset has no Ix1 Dot impl). v0: optional start vector over ALL columns.
int scanrs_multi_pca_irlba(scanrs_multi *mm, uint32_t nu, double tol, uint32_t max_iter, const double *v0, const scanrs_snoop *snoop,
                           double *u, double *s, double *v, uint32_t *mprod) {
    if (!u || !v) return SCANRS_ERR_ARGUMENT;
    std::vector<uint32_t> mp(mm ? mm->shards.size() : 0, 0);
    const int rc = multi_pca(mm, nu, snoop, u, s, v, [&](size_t i, scanrs_mat *h, const scanrs_snoop *sn, ShardOutputs &o, double *ui, double *si, double *vi) {
        const bool cols_sharded = mm->storage == SCANRS_CSC;
        const uint64_t n_loc = mm->bounds[i + 1] - mm->bounds[i];
        // scanrs_pca_irlba wants both factors: the replicated one of shards > 0 goes to a scratch array
        if (!ui) ui = o.out(ui, (size_t)(cols_sharded ? mm->rows : n_loc) * nu);
        if (!vi) vi = o.out(vi, (size_t)(cols_sharded ? n_loc : mm->cols) * nu);
        const double *v0i = v0 ? (cols_sharded ? v0 + mm->bounds[i] : v0) : nullptr;
        return scanrs_pca_irlba(h, nu, tol, max_iter, v0i, sn, ui, si, vi, &mp[i]);
    });
    if (mprod && !mp.empty()) *mprod = mp[0];
    return rc;
}

// Raw-count log normalisation without the centre / scale step (the only input irlba.rs takes).
int scanrs_multi_log_normalize(scanrs_multi *mm, double umi_count_sum, int log_fn, const uint32_t *size_factors) {
    if (!mm) return SCANRS_ERR_ARGUMENT;
    return fan_out(mm, [&](size_t i) {
        const uint32_t *sf = size_factors;
        if (sf && mm->storage == SCANRS_CSC) sf += mm->bounds[i];
        return scanrs_log_normalize(mm->shards[i], umi_count_sum, log_fn, sf);
    });
}

// ---- sSeq differential expression over the shards -----------------------------------------------------------------
// The calls of the handle (scanrs_sseq_params, scanrs_mat_group_sums, scanrs_sseq_de_backend) on every shard at once. The cells must
// be the sharded dimension: a genes x cells CSC matrix, or a cells x genes CSR one with transposed = 1 (every shard then goes through
// scanrs_mat_t). Each is one call under the collective frame above.
int scanrs_multi_sseq_params(scanrs_multi *mm, int transposed, double zeta_quintile, const uint64_t *cell_indices, uint64_t n_sel,
                             const double *umi_counts, double *size_factors, double *gene_means, double *gene_variances, uint8_t *use_genes,
                             double *gene_moment_phi, double *zeta_hat, double *delta, double *gene_phi) {
    if (!mm || !size_factors || !gene_means || !gene_variances || !use_genes || !gene_moment_phi || !zeta_hat || !delta || !gene_phi)
        return bad_argument("null argument");
    const uint64_t genes = transposed ? mm->cols : mm->rows, cells = transposed ? mm->rows : mm->cols;
    return collective(mm, transposed, nullptr, [&](size_t, scanrs_mat *h, const scanrs_snoop *, ShardOutputs &o) {
        return scanrs_sseq_params(h, zeta_quintile, cell_indices, n_sel, umi_counts, o.out(size_factors, cells), o.out(gene_means, genes),
                                  o.out(gene_variances, genes), o.out(use_genes, genes), o.out(gene_moment_phi, genes), o.out(zeta_hat, 1),
                                  o.out(delta, 1), o.out(gene_phi, genes));
    });
}

int scanrs_multi_group_sums(scanrs_multi *mm, int transposed, const int16_t *labels, uint32_t n_groups, uint64_t *sums, uint64_t *cells_per_group) {
    if (!mm || !labels || !sums) return bad_argument("null argument");
    if (n_groups == 0 || n_groups > SSEQ_MAX_GROUPS) return bad_argument("n_groups must be in 1 .. 8192");
    const uint64_t genes = transposed ? mm->cols : mm->rows;
    return collective(mm, transposed, nullptr, [&](size_t, scanrs_mat *h, const scanrs_snoop *, ShardOutputs &o) {
        return scanrs_mat_group_sums(h, labels, n_groups, o.out(sums, genes * n_groups), o.optional(cells_per_group));
    });
}

int scanrs_multi_sseq_de(scanrs_multi *mm, int transposed, const int16_t *labels, uint32_t n_groups, int mode, const double *size_factors,
                         const double *gene_means, const double *gene_phi, const uint8_t *use_genes, uint64_t big_count, int backend,
                         const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc,
                         double *mean_in, double *mean_out) {
    if (mode != 0 && mode != 1 && mode != 2)
        return bad_argument("mode must be 0 (one against the rest), 1 (group 0 against group 1) or 2 (each group against group 0)");
    if (backend != SCANRS_NB_EXACT_LOGSPACE && backend != SCANRS_NB_EXACT_RATIO)
        return bad_argument("backend must be SCANRS_NB_EXACT_LOGSPACE (0) or SCANRS_NB_EXACT_RATIO (1)");
    if (!mm || !labels || !size_factors || !gene_means || !gene_phi || !use_genes || !sums_in || !sums_out || !p || !p_adj || !log2fc || !mean_in ||
        !mean_out)
        return bad_argument("null argument");
    if (n_groups == 0 || n_groups > SSEQ_MAX_GROUPS) return bad_argument("n_groups must be in 1 .. 8192");
    const uint64_t genes = transposed ? mm->cols : mm->rows;
    const uint64_t total = genes * (mode == 0 ? n_groups : mode == 1 ? 1 : n_groups - 1);
    return collective(mm, transposed, snoop, [&](size_t, scanrs_mat *h, const scanrs_snoop *sn, ShardOutputs &o) {
        return scanrs_sseq_de_backend(h, labels, n_groups, mode, size_factors, gene_means, gene_phi, use_genes, big_count, backend, sn,
                                      o.out(sums_in, total), o.out(sums_out, total), o.out(p, total), o.out(p_adj, total), o.out(log2fc, total),
                                      o.out(mean_in, total), o.out(mean_out, total));
    });
}

// ---- sseq_de_pairs, merge_clusters and the medoids over the shards ------------------------------------------------------
// The collective calls of the handle (scanrs_*_sharded) under the same frame; the pair parameters and the trace are shard 0's alone.
int scanrs_multi_sseq_de_pairs(scanrs_multi *mm, int transposed, const int16_t *labels, uint32_t n_groups, const uint32_t *pair_a,
                               const uint32_t *pair_b, uint32_t n_pairs, double zeta_quintile, uint64_t big_count, int backend,
                               const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc,
                               double *mean_in, double *mean_out, scanrs_sseq_pair_params *params) {
    if (backend != SCANRS_NB_EXACT_LOGSPACE && backend != SCANRS_NB_EXACT_RATIO)
        return bad_argument("backend must be SCANRS_NB_EXACT_LOGSPACE (0) or SCANRS_NB_EXACT_RATIO (1)");
    if (!(zeta_quintile >= 0.0 && zeta_quintile <= 1.0)) return bad_argument("zeta_quintile must be in [0, 1]");
    if (!mm || !labels || (n_pairs && (!pair_a || !pair_b)) || !sums_in || !sums_out || !p || !p_adj || !log2fc || !mean_in || !mean_out)
        return bad_argument("null argument");
    if (n_pairs == 0) return bad_argument("n_pairs must be at least 1");
    if (n_groups == 0 || n_groups > SSEQ_MAX_GROUPS) return bad_argument("n_groups must be in 1 .. 8192");
    const uint64_t genes = transposed ? mm->cols : mm->rows;
    const uint64_t total = genes * n_pairs;
    return collective(mm, transposed, snoop, [&](size_t, scanrs_mat *h, const scanrs_snoop *sn, ShardOutputs &o) {
        return scanrs_sseq_de_pairs_sharded(h, labels, n_groups, pair_a, pair_b, n_pairs, zeta_quintile, big_count, backend, sn, o.out(sums_in, total),
                                            o.out(sums_out, total), o.out(p, total), o.out(p_adj, total), o.out(log2fc, total), o.out(mean_in, total),
                                            o.out(mean_out, total), o.optional(params));
    });
}

int scanrs_multi_cluster_medoids(scanrs_multi *mm, int transposed, const double *pca, uint32_t ld, uint32_t d, const int16_t *labels, uint32_t k,
                                 double *centers) {
    if (!mm) return bad_argument("null handle");
    const uint64_t cells = transposed ? mm->rows : mm->cols;
    if (cells && (!pca || !labels || (!centers && d))) return bad_argument("null argument");
    if (ld < d) return bad_argument("ld must be at least d");
    return collective(mm, transposed, nullptr, [&](size_t, scanrs_mat *h, const scanrs_snoop *, ShardOutputs &o) {
        return scanrs_cluster_medoids_sharded(h, pca, 0, ld, d, labels, k, o.out(centers, (size_t)k * d));
    });
}

int scanrs_multi_merge_clusters(scanrs_multi *mm, int transposed, const double *pca, uint32_t ld, uint32_t d, const int16_t *labels,
                                int16_t *labels_out, const scanrs_snoop *snoop, scanrs_merge_trace *trace) {
    if (!mm) return bad_argument("null handle");
    const uint64_t cells = transposed ? mm->rows : mm->cols;
    if (cells && (!pca || !labels || !labels_out)) return bad_argument("null argument");
    if (trace && trace->capacity && (!trace->leaf0 || !trace->leaf1 || !trace->n_de || !trace->min_p_adj)) return bad_argument("trace arrays are null");
    if (ld < d) return bad_argument("ld must be at least d");
    return collective(mm, transposed, snoop, [&](size_t, scanrs_mat *h, const scanrs_snoop *sn, ShardOutputs &o) {
        return scanrs_merge_clusters_sharded(h, pca, 0, ld, d, labels, o.out(labels_out, cells), sn, o.optional(trace));
    });
}

// ---- knn over the shards (nn.rs:38-83) -----------------------------------------------------------------------------------
namespace {
// the points of shard i for a scanrs_*_sharded search: the caller's host array over all cells, or the factor along the sharded
// dimension that the shard's last PCA left on its device. search(handle, points, points_is_device, ld, d, first cell of the shard)
int multi_search_points(scanrs_multi *mm, const char *name, const double *points, uint32_t ld, uint32_t d,
                        const std::function<int(scanrs_mat *, const double *, int, uint32_t, uint32_t, uint64_t)> &search) {
    const int transposed = mm->storage == SCANRS_CSR;
    return collective(mm, transposed, nullptr, [&](size_t i, scanrs_mat *h, const scanrs_snoop *, ShardOutputs &) {
        const uint64_t lo = mm->bounds[i], n_loc = mm->bounds[i + 1] - lo;
        if (points) return search(h, points, 0, ld, d, lo);
        const double *du = nullptr, *dv = nullptr;
        uint32_t ldu = 0, ldv = 0, kk = 0;
        if (const int rc = scanrs_pca_result_device(mm->shards[i], &du, &ldu, &dv, &ldv, &kk)) return rc; // "no PCA result on this handle yet"
        const Storage::PcaDev &r = mm->shards[i]->st->pca_dev;
        const uint64_t rows = transposed ? r.rows_u : r.rows_v;
        if (rows != n_loc) {
            set_error("%s: the factor along the sharded dimension is not kept per shard (%llu rows on the device for %llu cells): pass the scores as a host array",
                      name, (unsigned long long)rows, (unsigned long long)n_loc);
            return (int)SCANRS_ERR_ARGUMENT;
        }
        return search(h, transposed ? du : dv, 1, transposed ? ldu : ldv, kk, lo);
    });
}
} // namespace

// scanrs_knn_sharded on every shard at once. The cells are the sharded dimension (the columns of a CSC matrix, the rows of a CSR
// one, which goes through its transposed view); every shard writes its own rows of the caller's arrays. points == NULL: every shard
// searches the factor along the sharded dimension that its last scanrs_multi_pca_bk / _rand left on its device (V of a genes x cells
// CSC matrix, U of a cells x genes CSR one), where that factor has the shard's own rows.
int scanrs_multi_knn(scanrs_multi *mm, const double *points, uint32_t ld, uint32_t d, uint32_t k, uint32_t *out, double *sq_dist) {
    if (!mm) return bad_argument("null handle");
    if (mm->bounds.back() && k && !out) return bad_argument("null argument");
    return multi_search_points(mm, "multi_knn", points, ld, d, [&](scanrs_mat *h, const double *p, int on_device, uint32_t ldp, uint32_t dp, uint64_t lo) {
        return scanrs_knn_sharded(h, p, on_device, ldp, dp, k, out ? out + lo * k : nullptr, sq_dist ? sq_dist + lo * k : nullptr);
    });
}

// scanrs_nearest_neighbors_sharded on every shard at once (knn.rs:112-166): the conventions of scanrs_multi_knn, points ==
// NULL included.
int scanrs_multi_nearest_neighbors(scanrs_multi *mm, const double *points, uint32_t ld, uint32_t d, uint32_t k, int distance_type,
                                   uint32_t *indices, double *distances) {
    if (!mm) return bad_argument("null handle");
    if (mm->bounds.back() && k && (!indices || !distances)) return bad_argument("null argument");
    return multi_search_points(mm, "multi_nearest_neighbors", points, ld, d,
                               [&](scanrs_mat *h, const double *p, int on_device, uint32_t ldp, uint32_t dp, uint64_t lo) {
                                   return scanrs_nearest_neighbors_sharded(h, p, on_device, ldp, dp, k, distance_type,
                                                                           indices ? indices + lo * k : nullptr,
                                                                           distances ? distances + lo * k : nullptr);
                               });
}

// ---- select_rows / select_cols / partition_on_thresholds over the shards -------------------------------------------------
// The collective entry points of the handle (scanrs_mat_*_sharded) on every shard at once. Every result is a new scanrs_multi on the
// same devices with as many shards, the ranges its shards ended up with (nothing is rebalanced), and a group and communicators of its
// own: the source and its results may be freed in either order.
namespace {

// takes over `made` (one result handle per shard of src, bound to src's communicators); on failure everything in it is freed
int multi_adopt(scanrs_multi *src, std::vector<scanrs_mat *> &made, scanrs_multi **out) {
    const int rc = guard([&] {
        auto mm = std::make_unique<scanrs_multi>();
        const uint32_t n = (uint32_t)made.size();
        mm->storage = src->storage;
        mm->devices = src->devices;
        mm->bounds.assign(n + 1, 0);
        uint64_t outer_all = 0, inner = 0;
        for (uint32_t i = 0; i < n; i++) {
            uint64_t begin = 0, all = 0, r = 0, c = 0;
            if (scanrs_mat_shard_info(made[i], nullptr, nullptr, &begin, &all) != SCANRS_OK || scanrs_mat_shape(made[i], &r, &c) != SCANRS_OK)
                throw Failure{SCANRS_ERR_ARGUMENT};
            const uint64_t local = mm->storage == SCANRS_CSR ? r : c;
            if (begin != mm->bounds[i] || (i && all != outer_all)) fail(SCANRS_ERR_DEVICE, "internal: the result shards do not tile the outer dimension");
            mm->bounds[i + 1] = begin + local;
            outer_all = all;
            inner = mm->storage == SCANRS_CSR ? c : r;
        }
        if (mm->bounds[n] != outer_all) fail(SCANRS_ERR_DEVICE, "internal: the result shards do not tile the outer dimension");
        mm->rows = mm->storage == SCANRS_CSR ? outer_all : inner;
        mm->cols = mm->storage == SCANRS_CSR ? inner : outer_all;
        mm->group = local_group_make(n);
        for (uint32_t i = 0; i < n; i++) mm->comms.push_back(comm_make_local(mm->group, i));
        for (uint32_t i = 0; i < n; i++)
            if (scanrs_mat_set_shard_comm(made[i], mm->comms[i], i, n, mm->bounds[i], outer_all) != SCANRS_OK) {
                for (auto *c : mm->comms) scanrs_comm_free(c);
                throw Failure{SCANRS_ERR_ARGUMENT};
            }
        mm->shards = std::move(made);
        made.clear();
        *out = mm.release();
    });
    return rc == SCANRS_OK ? rc : failed(rc, [&] { free_shards(src, made); });
}

int multi_select(scanrs_multi *mm, bool rows_axis, const uint64_t *idx, uint64_t n_idx, scanrs_multi **out) {
    if (!out) return bad_argument("null output handle");
    *out = nullptr;
    if (!mm) return bad_argument("null handle");
    std::vector<scanrs_mat *> made(mm->shards.size(), nullptr);
    const int rc = fan_out(mm, [&](size_t i) {
        return rows_axis ? scanrs_mat_select_rows_sharded(mm->shards[i], idx, n_idx, &made[i]) : scanrs_mat_select_cols_sharded(mm->shards[i], idx, n_idx, &made[i]);
    });
    if (rc != SCANRS_OK) return failed(rc, [&] { free_shards(mm, made); });
    return multi_adopt(mm, made, out);
}

} // namespace

// ---- the statistics over a list of columns over the shards ----------------------------------------------------------------
// The collective calls of the handle (scanrs_mat_sum_rows_u64_sharded and kin) under the collective frame: global lists, complete
// outputs on every shard.
namespace {

// f(handle, out_a, out_b, snoop) on every shard; n_res: the entries of an output (out_b: null unless `two`; its type follows out_a's)
extern "C++" template <typename T, typename F>
int multi_subset(scanrs_multi *mm, int transposed, T *out_a, std::common_type_t<T> *out_b, bool two, uint64_t n_res, const scanrs_snoop *snoop, F &&f) {
    if (!mm) return bad_argument("null handle");
    if (n_res && (!out_a || (two && !out_b))) return bad_argument("null argument");
    return collective(mm, transposed, snoop, [&](size_t, scanrs_mat *h, const scanrs_snoop *sn, ShardOutputs &o) {
        return f(h, o.out(out_a, n_res), two ? o.out(out_b, n_res) : nullptr, sn);
    });
}
uint64_t view_rows(const scanrs_multi *mm, int transposed) { return !mm ? 0 : transposed ? mm->cols : mm->rows; }

} // namespace

int scanrs_multi_sum_rows_u64(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, uint64_t *out) {
    return multi_subset(mm, transposed, out, nullptr, false, view_rows(mm, transposed), nullptr, [&](scanrs_mat *h, uint64_t *a, uint64_t *, const scanrs_snoop *) {
        return scanrs_mat_sum_rows_u64_sharded(h, cols, n, a);
    });
}
int scanrs_multi_sum_rows_f64(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, double *out) {
    return multi_subset(mm, transposed, out, nullptr, false, view_rows(mm, transposed), nullptr, [&](scanrs_mat *h, double *a, double *, const scanrs_snoop *) {
        return scanrs_mat_sum_rows_f64_sharded(h, cols, n, a);
    });
}
int scanrs_multi_sum_cols_u64(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, uint64_t *out) {
    return multi_subset(mm, transposed, out, nullptr, false, n, nullptr, [&](scanrs_mat *h, uint64_t *a, uint64_t *, const scanrs_snoop *) {
        return scanrs_mat_sum_cols_u64_sharded(h, cols, n, a);
    });
}
int scanrs_multi_sum_cols_f64(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, double *out) {
    return multi_subset(mm, transposed, out, nullptr, false, n, nullptr, [&](scanrs_mat *h, double *a, double *, const scanrs_snoop *) {
        return scanrs_mat_sum_cols_f64_sharded(h, cols, n, a);
    });
}
int scanrs_multi_sum_rows_dual_u64(scanrs_multi *mm, int transposed, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                   const scanrs_snoop *snoop, uint64_t *out1, uint64_t *out2) {
    return multi_subset(mm, transposed, out1, out2, true, view_rows(mm, transposed), snoop, [&](scanrs_mat *h, uint64_t *a, uint64_t *b, const scanrs_snoop *sn) {
        return scanrs_mat_sum_rows_dual_u64_sharded(h, cols1, n1, cols2, n2, sn, a, b);
    });
}
int scanrs_multi_sum_rows_dual_f64(scanrs_multi *mm, int transposed, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                   const scanrs_snoop *snoop, double *out1, double *out2) {
    return multi_subset(mm, transposed, out1, out2, true, view_rows(mm, transposed), snoop, [&](scanrs_mat *h, double *a, double *b, const scanrs_snoop *sn) {
        return scanrs_mat_sum_rows_dual_f64_sharded(h, cols1, n1, cols2, n2, sn, a, b);
    });
}
int scanrs_multi_mean_rows(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, double *out) {
    return multi_subset(mm, transposed, out, nullptr, false, view_rows(mm, transposed), nullptr, [&](scanrs_mat *h, double *a, double *, const scanrs_snoop *) {
        return scanrs_mat_mean_rows_sharded(h, cols, n, a);
    });
}
int scanrs_multi_mean_var_rows(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, double *mean, double *var) {
    return multi_subset(mm, transposed, mean, var, true, view_rows(mm, transposed), nullptr, [&](scanrs_mat *h, double *a, double *b, const scanrs_snoop *) {
        return scanrs_mat_mean_var_rows_sharded(h, cols, n, a, b);
    });
}

int scanrs_multi_shape(const scanrs_multi *mm, uint64_t *rows, uint64_t *cols, uint64_t *nnz, int *storage) {
    if (!mm) return bad_argument("null handle");
    if (rows) *rows = mm->rows;
    if (cols) *cols = mm->cols;
    if (storage) *storage = mm->storage;
    if (nnz) {
        *nnz = 0;
        for (auto *h : mm->shards) {
            uint64_t x = 0;
            if (const int rc = scanrs_mat_nnz(h, &x)) return rc;
            *nnz += x;
        }
    }
    return SCANRS_OK;
}

int scanrs_multi_to_csmat(scanrs_multi *mm, uint64_t *indptr, uint32_t *indices, uint32_t *values) {
    if (!mm || !indptr) return bad_argument("null argument");
    const size_t n = mm->shards.size();
    std::vector<uint64_t> first(n + 1, 0); // the place of every shard's first nonzero in the whole matrix
    for (size_t i = 0; i < n; i++) {
        uint64_t x = 0;
        if (const int rc = scanrs_mat_nnz(mm->shards[i], &x)) return rc;
        first[i + 1] = first[i] + x;
    }
    if (first[n] && (!indices || !values)) return bad_argument("null indices/values");
    indptr[mm->bounds[n]] = first[n];
    return fan_out(mm, [&](size_t i) {
        const uint64_t lo = mm->bounds[i], hi = mm->bounds[i + 1];
        std::vector<uint64_t> ip(hi - lo + 1);
        const bool some = first[i + 1] > first[i];
        if (const int rc = scanrs_mat_to_csmat(mm->shards[i], ip.data(), some ? indices + first[i] : nullptr, some ? values + first[i] : nullptr)) return rc;
        for (uint64_t o = lo; o < hi; o++) indptr[o] = ip[o - lo] + first[i];
        return (int)SCANRS_OK;
    });
}

int scanrs_multi_select_rows(scanrs_multi *mm, const uint64_t *idx, uint64_t n_idx, scanrs_multi **out) { return multi_select(mm, true, idx, n_idx, out); }
int scanrs_multi_select_cols(scanrs_multi *mm, const uint64_t *idx, uint64_t n_idx, scanrs_multi **out) { return multi_select(mm, false, idx, n_idx, out); }

int scanrs_multi_partition_on_thresholds(scanrs_multi *mm, const double *row_threshold, const double *col_threshold, scanrs_multi **filtered,
                                         scanrs_multi **residual, uint64_t *selected_rows, uint64_t *n_selected_rows, uint64_t *selected_cols,
                                         uint64_t *n_selected_cols) {
    if (filtered) *filtered = nullptr;
    if (residual) *residual = nullptr;
    if (!mm) return bad_argument("null handle");
    if (!selected_rows || !n_selected_rows || !selected_cols || !n_selected_cols) return bad_argument("null argument");
    const size_t n = mm->shards.size();
    std::vector<scanrs_mat *> made_f(n, nullptr), made_r(n, nullptr);
    int rc = collective(mm, 0, nullptr, [&](size_t i, scanrs_mat *h, const scanrs_snoop *, ShardOutputs &o) {
        // every shard computes the same complete lists
        return scanrs_mat_partition_on_thresholds_sharded(h, row_threshold, col_threshold, filtered ? &made_f[i] : nullptr, residual ? &made_r[i] : nullptr,
                                                          o.out(selected_rows, mm->rows), o.out(n_selected_rows, 1), o.out(selected_cols, mm->cols),
                                                          o.out(n_selected_cols, 1));
    });
    if (rc != SCANRS_OK)
        return failed(rc, [&] {
            free_shards(mm, made_f);
            free_shards(mm, made_r);
        });
    scanrs_multi *hf = nullptr, *hr = nullptr;
    if (filtered) rc = multi_adopt(mm, made_f, &hf);
    if (rc == SCANRS_OK && residual) rc = multi_adopt(mm, made_r, &hr);
    if (rc != SCANRS_OK)
        return failed(rc, [&] {
            scanrs_multi_free(hf);
            free_shards(mm, made_r);
        });
    if (filtered) *filtered = hf;
    if (residual) *residual = hr;
    return SCANRS_OK;
}

// ---- gather_outer / rebalance: outer vectors move between shards -----------------------------------------------------------
// "The outer vectors idx[0 .. n) of the whole matrix, in that order, as a freshly balanced scanrs_multi": the identity list is a
// rebalance, another shard count or other devices a re-sharding. The result equals scanrs_multi_create of the selected triplet, and no
// nonzero crosses the host link:
//   plan    every SOURCE shard sends the indptr of its own vectors to the host; regather_host_plan (the code of scanrs_host_plan_gather)
//           makes the selected matrix's indptr, cuts it with scanrs_plan_shards and counts `moved`;
//   pull    every DESTINATION uploads its slice of the list, finds each vector's length and place in the sources' indptr arrays, scans
//           the lengths into its own indptr and copies the entries tile by tile out of the sources' arrays, in place (regather.hip);
//   finish  the handle adopts the arrays as they are and is finished as scanrs_mat_create finishes one: the largest count, the work
//           items, its communicator and range.
// The phases are separate fan_outs (the join of the shard threads is the barrier, a failing shard ends its phase for all); no wait
// inside a phase depends on another shard, and the source's arrays are only read.
} // extern "C"

namespace {

int gather_outer(scanrs_multi *src, const uint64_t *idx, uint64_t n_idx, uint32_t n_shards, const int *devices, scanrs_multi **out) {
    if (!out) return bad_argument("out: null output handle");
    *out = nullptr;
    if (!src) return bad_argument("mm: null handle");
    const uint32_t n_src = (uint32_t)src->shards.size();
    const uint64_t n_outer = src->bounds.back(), n_inner = src->storage == SCANRS_CSR ? src->cols : src->rows;
    std::unique_ptr<scanrs_multi> mm;
    int rc = guard([&] {
        // everything that can be refused is refused here, before any device work
        check_shard_count(n_shards, "n_shards: 1 <= n_shards <= 16 is required (%u given)");
        if (n_src > REGATHER_MAX_SHARDS) fail(SCANRS_ERR_ARGUMENT, "mm: a source of more than 16 shards is not served");
        regather_check_list(idx, n_idx, n_outer);
        if (n_outer >= 0x7FFFFFFFull || n_inner >= 0x7FFFFFFFull) fail(SCANRS_ERR_SHAPE, "gather_outer needs dimensions below 2^31 - 1");
        for (const scanrs_mat *h : src->shards) {
            if (!h || h->transposed || !map_is_raw(h))
                fail(SCANRS_ERR_ARGUMENT, "gather_outer: the handle's map is not the identity (a scaling or a function has been composed); call scanrs_mat_reset_map first");
            if (h->off_rank)
                fail(SCANRS_ERR_ARGUMENT, "gather_outer: the handle has a low-rank offset (center / scale_and_center / normalize); call scanrs_mat_reset_map first");
        }
        mm = std::make_unique<scanrs_multi>();
        mm->rows = src->storage == SCANRS_CSR ? n_idx : src->rows;
        mm->cols = src->storage == SCANRS_CSR ? src->cols : n_idx;
        mm->storage = src->storage;
        bind_devices(mm.get(), n_shards, devices);
        for (uint32_t d = 0; d < n_shards; d++)
            for (uint32_t s = 0; s < n_src; s++) enable_peer(mm->devices[d], src->devices[s]);
        mm->bounds.assign(n_shards + 1, 0);
        mm->gather = std::make_shared<scanrs_multi::GatherInfo>();
        mm->gather->n_src = n_src;
        mm->gather->moved.assign((size_t)n_src * n_shards, 0);
        mm->gather->host_bytes.assign(n_shards, 0);
    });
    const auto give_up = [&] { scanrs_multi_free(mm.release()); }; // (of a null handle: nothing)
    if (rc != SCANRS_OK) return failed(rc, give_up);
    scanrs_multi *raw = mm.get();
    scanrs_multi::GatherInfo &info = *raw->gather;
    jump_tables_prefetch(); // as scanrs_mat_create does
    const auto t_plan = std::chrono::steady_clock::now();

    // plan, 1: the lengths. Every source shard's indptr goes down (8 bytes per vector), charged to destination s mod n_shards.
    std::vector<std::vector<uint64_t>> src_ip(n_src);
    rc = fan_out(src, [&](size_t s) {
        return guard([&] {
            need_device();
            Storage &st = *src->shards[s]->st;
            CurrentHandle cur(&st);
            const SparseCopy &cp = st.primary;
            if (cp.n_outer != src->bounds[s + 1] - src->bounds[s]) fail(SCANRS_ERR_DEVICE, "internal: a source shard does not hold its range");
            src_ip[s].assign(cp.n_outer + 1, 0);
            SCANRS_D2H(src_ip[s].data(), cp.indptr.p, (cp.n_outer + 1) * 8, st.stream);
            SCANRS_SYNC(st.stream); // whatever was queued on the source before this call is done before a destination reads its arrays
        });
    });
    // plan, 2: on the host, the code of scanrs_host_plan_gather
    std::vector<uint64_t> tip(n_idx + 1, 0);
    if (rc == SCANRS_OK)
        rc = guard([&] {
            std::vector<uint64_t> gip(n_outer + 1, 0);
            uint64_t first = 0;
            for (uint32_t s = 0; s < n_src; s++) {
                const uint64_t lo = src->bounds[s], n = src->bounds[s + 1] - lo;
                for (uint64_t o = 0; o <= n; o++) gip[lo + o] = first + src_ip[s][o];
                first += src_ip[s][n];
                info.host_bytes[s % n_shards] += 8 * (n + 1);
                std::vector<uint64_t>().swap(src_ip[s]);
            }
            regather_host_plan(gip.data(), n_outer, src->bounds.data(), n_src, idx, n_idx, n_shards, tip.data(), raw->bounds.data(), info.moved.data());
        });
    info.bounds = raw->bounds;
    const uint64_t plan_us = (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_plan).count();

    // pull: every destination reads its vectors out of the sources' arrays
    if (rc == SCANRS_OK)
        rc = fan_out(raw, [&](size_t d) {
            return guard([&] {
                need_device();
                const uint64_t lo = raw->bounds[d], n_loc = raw->bounds[d + 1] - lo, nnz = tip[lo + n_loc] - tip[lo];
                Storage &st = *make_shard(raw, d, raw->storage == SCANRS_CSR ? n_loc : raw->rows, raw->storage == SCANRS_CSR ? raw->cols : n_loc)->st;
                CurrentHandle cur(&st);
                st.regather_us[0] = plan_us; // (the plan is one phase for all shards)
                PhaseClock clock(st.regather_us[1]);
                RegatherSources from;
                from.n = n_src;
                for (uint32_t s = 0; s < n_src; s++) {
                    const SparseCopy &cp = src->shards[s]->st->primary;
                    from.bounds[s] = src->bounds[s];
                    from.nnz[s] = cp.nnz;
                    from.indptr[s] = cp.indptr.p;
                    from.indices[s] = cp.indices.p;
                    from.values[s] = cp.values.p;
                }
                from.bounds[n_src] = n_outer;
                SparseCopy &cp = st.primary;
                cp.n_outer = n_loc;
                cp.n_inner = n_inner;
                cp.nnz = nnz;
                std::vector<uint32_t> list(n_loc);
                for (uint64_t j = 0; j < n_loc; j++) list[j] = (uint32_t)idx[lo + j];
                DevBuf<uint32_t> d_list(std::max<uint64_t>(1, n_loc));
                DevBuf<uint64_t> d_place(std::max<uint64_t>(1, n_loc));
                if (n_loc) SCANRS_HIP(hipMemcpyAsync(d_list.p, list.data(), n_loc * 4, hipMemcpyHostToDevice, st.stream));
                cp.indptr.alloc(n_loc + 1);
                launch_regather_len(st.stream, from, d_list.p, n_loc, reinterpret_cast<unsigned long long *>(cp.indptr.p), d_place.p);
                select_scan_offsets(st.stream, reinterpret_cast<unsigned long long *>(cp.indptr.p), n_loc);
                // the one value that comes back: the device's lengths add up to the plan's
                const uint64_t got = SCANRS_D2H_VALUE(cp.indptr.p + n_loc, st.stream);
                if (got != nnz)
                    fail(SCANRS_ERR_DEVICE, "internal: the gathered lengths (%llu entries) do not match the plan (%llu)", (unsigned long long)got, (unsigned long long)nnz);
                info.host_bytes[d] += 4 * n_loc + 8;
                cp.indices.alloc(std::max<uint64_t>(1, nnz));
                cp.values.alloc(std::max<uint64_t>(1, nnz));
                launch_regather_pull(st.stream, from, cp.indptr.p, d_place.p, n_loc, nnz, cp.indices.p, cp.values.p);
                SCANRS_SYNC(st.stream); // the list and the places are released on return
            });
        });

    // finish: what scanrs_mat_create leaves behind on a validated copy, then the shard's communicator and range
    if (rc == SCANRS_OK)
        rc = fan_out(raw, [&](size_t d) {
            return guard([&] {
                Storage &st = *raw->shards[d]->st;
                CurrentHandle cur(&st);
                PhaseClock clock(st.regather_us[2]);
                finish_shard(raw, d, st.primary, true, n_idx, [] {});
            });
        });

    if (rc != SCANRS_OK) return failed(rc, give_up);
    *out = mm.release();
    return SCANRS_OK;
}

} // namespace

extern "C" {

int scanrs_multi_gather_outer(scanrs_multi *mm, const uint64_t *idx, uint64_t n_idx, uint32_t n_shards, const int *devices, scanrs_multi **out) {
    return gather_outer(mm, idx, n_idx, n_shards, devices, out);
}

int scanrs_multi_rebalance(scanrs_multi *mm, uint32_t n_shards, const int *devices, scanrs_multi **out) {
    if (!out) return bad_argument("out: null output handle");
    *out = nullptr;
    if (!mm) return bad_argument("mm: null handle");
    std::vector<uint64_t> all;
    const int rc = guard([&] {
        all.resize(mm->bounds.back());
        for (uint64_t o = 0; o < all.size(); o++) all[o] = o;
    });
    if (rc != SCANRS_OK) return rc;
    if (n_shards == 0) return gather_outer(mm, all.data(), all.size(), (uint32_t)mm->shards.size(), mm->devices.data(), out);
    return gather_outer(mm, all.data(), all.size(), n_shards, devices, out);
}

int scanrs_multi_balance(const scanrs_multi *mm, uint64_t *shard_nnz, double *imbalance) {
    if (!mm) return bad_argument("mm: null handle");
    uint64_t total = 0, most = 0;
    for (size_t i = 0; i < mm->shards.size(); i++) {
        uint64_t x = 0;
        if (const int rc = scanrs_mat_nnz(mm->shards[i], &x)) return rc;
        if (shard_nnz) shard_nnz[i] = x;
        total += x;
        most = std::max(most, x);
    }
    if (imbalance) *imbalance = total ? (double)most * (double)mm->shards.size() / (double)total : 1.0; // (no nonzeros: nothing to balance)
    return SCANRS_OK;
}

int scanrs_multi_gather_info(const scanrs_multi *mm, uint32_t *n_src, uint64_t *bounds, uint64_t *moved, uint64_t *host_bytes) {
    if (!mm) return bad_argument("mm: null handle");
    if (!mm->gather) return bad_argument("gather_info: this scanrs_multi was not made by scanrs_multi_gather_outer or scanrs_multi_rebalance");
    const scanrs_multi::GatherInfo &info = *mm->gather;
    if (n_src) *n_src = info.n_src;
    if (bounds) std::copy(info.bounds.begin(), info.bounds.end(), bounds);
    if (moved) std::copy(info.moved.begin(), info.moved.end(), moved);
    if (host_bytes) std::copy(info.host_bytes.begin(), info.host_bytes.end(), host_bytes);
    return SCANRS_OK;
}

// ---- to_adaptive of the whole matrix, in either orientation (mat.rs:92-124 backwards, hdf5-io/src/matrix.rs:119-192) --------
// STORED: every shard runs the encoders on its own primary copy; one table in global order over one pair of host arenas per shard.
// INNER, the inverse of scanrs_multi_create_adaptive_inner: one vector per inner position, spanning all shards. An encoding of a
// vector's slice cannot be concatenated, so the vectors are made whole on a device first:
//   copies  every shard settles its transposed copy T_s (n_inner vectors over its own outer positions) and sends T_s's indptr down;
//   plan    export_host_plan (the code of scanrs_host_plan_export): the whole matrix's inner-major indptr from the summed counts, cut
//           by scanrs_plan_shards into one slab of inner positions per shard, and `moved`;
//   pull    destination d assembles the CSR of slab d over all outer positions out of the sources' T_s, in place (export_multi.hip);
//   encode  the encoders run on the slab as on any SparseCopy, the two arenas come down, the slab goes.
// The phases are separate fan_outs (the join of the shard threads is the barrier, a failing shard ends its phase for all); no wait
// inside a phase depends on another shard, and the sources' arrays are only read.
} // extern "C"

namespace {

using ExportPtr = std::unique_ptr<scanrs_adaptive_export, void (*)(scanrs_adaptive_export *)>;

int multi_to_adaptive(scanrs_multi *mm, int major, int force_kind, scanrs_adaptive_export **out) {
    const uint32_t n = (uint32_t)mm->shards.size();
    const uint64_t outer_global = mm->bounds.back(), n_inner = mm->storage == SCANRS_CSR ? mm->cols : mm->rows;
    ExportPtr e(nullptr, scanrs_adaptive_export_free);
    std::vector<uint64_t> slab_bounds(n + 1, 0), moved((size_t)n * n, 0), arena_bytes(n, 0);
    const auto shard_storage = [&](size_t i) -> Storage & {
        need_device();
        Storage &st = *mm->shards[i]->st;
        if (st.primary.n_outer != mm->bounds[i + 1] - mm->bounds[i] || st.primary.n_inner != n_inner)
            fail(SCANRS_ERR_DEVICE, "internal: a shard does not hold its range");
        return st;
    };

    if (major == SCANRS_EXPORT_STORED) {
        int rc = guard([&] { e.reset(adaptive_export_new(outer_global, n)); });
        slab_bounds = mm->bounds;
        if (rc == SCANRS_OK)
            rc = fan_out(mm, [&](size_t i) {
                return guard([&] {
                    Storage &st = shard_storage(i);
                    CurrentHandle cur(&st);
                    st.export_us[0] = st.export_us[1] = st.export_us[2] = 0;
                    PhaseClock clock(st.export_us[2]);
                    adaptive_export_encode(e.get(), (uint32_t)i, st, st.primary, force_kind, mm->bounds[i], &arena_bytes[i]);
                    moved[i * n + i] = st.primary.nnz;
                });
            });
        if (rc != SCANRS_OK) return rc;
        if (const int rc2 = guard([&] { adaptive_export_finish(e.get(), slab_bounds, moved, arena_bytes); })) return rc2;
        *out = e.release();
        return SCANRS_OK;
    }

    // copies: T_s on every shard, its indptr to the host (8 (n_inner + 1) bytes: all that crosses the host link before the arenas)
    const auto t_plan = std::chrono::steady_clock::now();
    std::vector<uint64_t> counts, tip(n_inner + 1, 0);
    std::vector<const SparseCopy *> tcopy(n, nullptr);
    int rc = guard([&] {
        if (n > REGATHER_MAX_SHARDS) fail(SCANRS_ERR_ARGUMENT, "mm: a scanrs_multi of more than 16 shards is not served");
        if (outer_global > 0xFFFFFFFFull || n_inner > 0xFFFFFFFFull) fail(SCANRS_ERR_SHAPE, "dimensions must fit in u32 (AdaptiveVec limit)");
        for (uint32_t d = 0; d < n; d++)
            for (uint32_t s = 0; s < n; s++) enable_peer(mm->devices[d], mm->devices[s]);
        counts.assign((size_t)n * n_inner, 0);
    });
    if (rc == SCANRS_OK)
        rc = fan_out(mm, [&](size_t s) {
            return guard([&] {
                Storage &st = shard_storage(s);
                CurrentHandle cur(&st);
                st.export_us[0] = st.export_us[1] = st.export_us[2] = 0;
                const SparseCopy &t = st.copy_with_outer_rows(st.storage != SCANRS_CSR); // built as the products build it, and kept
                if (t.n_outer != n_inner || t.n_inner != st.primary.n_outer || t.nnz != st.primary.nnz)
                    fail(SCANRS_ERR_DEVICE, "internal: a shard's transposed copy does not match its range");
                std::vector<uint64_t> ip(n_inner + 1, 0);
                SCANRS_D2H(ip.data(), t.indptr.p, (n_inner + 1) * 8, st.stream);
                SCANRS_SYNC(st.stream); // whatever was queued on the source before this call is done before a destination reads its arrays
                if (ip[n_inner] != t.nnz) fail(SCANRS_ERR_DEVICE, "internal: a shard's transposed indptr does not end at its nonzeros");
                for (uint64_t g = 0; g < n_inner; g++) counts[s * n_inner + g] = ip[g + 1] - ip[g];
                tcopy[s] = &t;
            });
        });
    // plan: on the host, the code of scanrs_host_plan_export
    if (rc == SCANRS_OK)
        rc = guard([&] {
            export_host_plan(counts.data(), n, n_inner, n, tip.data(), slab_bounds.data(), moved.data());
            std::vector<uint64_t>().swap(counts);
            e.reset(adaptive_export_new(n_inner, n));
        });
    const uint64_t plan_us = (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_plan).count();

    // pull: every destination assembles the CSR of its slab out of the sources' transposed copies
    std::vector<SparseCopy> slab(n);
    if (rc == SCANRS_OK)
        rc = fan_out(mm, [&](size_t d) {
            return guard([&] {
                Storage &st = *mm->shards[d]->st;
                CurrentHandle cur(&st);
                st.export_us[0] = plan_us; // (the plan is one phase for all shards)
                PhaseClock clock(st.export_us[1]);
                RegatherSources from;
                from.n = n;
                for (uint32_t s = 0; s < n; s++) {
                    from.bounds[s] = mm->bounds[s];
                    from.nnz[s] = tcopy[s]->nnz;
                    from.indptr[s] = tcopy[s]->indptr.p;
                    from.indices[s] = tcopy[s]->indices.p;
                    from.values[s] = tcopy[s]->values.p;
                }
                from.bounds[n] = outer_global;
                const uint64_t g0 = slab_bounds[d], nv = slab_bounds[d + 1] - g0, nnz = tip[g0 + nv] - tip[g0];
                SparseCopy &cp = slab[d];
                cp.n_outer = nv;
                cp.n_inner = outer_global;
                cp.nnz = nnz;
                DevBuf<uint64_t> d_start;
                try {
                    cp.indptr.alloc(nv + 1);
                    cp.indices.alloc(std::max<uint64_t>(1, nnz));
                    cp.values.alloc(std::max<uint64_t>(1, nnz));
                    d_start.alloc(std::max<uint64_t>(1, (uint64_t)(n + 1) * nv));
                } catch (const Failure &f) {
                    if (f.code != SCANRS_ERR_DEVICE) throw;
                    const std::string why = scanrs_last_error();
                    fail(SCANRS_ERR_DEVICE, "shard %zu cannot hold its export slab (%llu vectors, %llu nonzeros: %llu bytes) beside what the library holds: %s", d,
                         (unsigned long long)nv, (unsigned long long)nnz, (unsigned long long)(8 * nnz + 8 * (nv + 1) * (n + 2)), why.c_str());
                }
                launch_export_len(st.stream, from, g0, nv, reinterpret_cast<unsigned long long *>(cp.indptr.p));
                select_scan_offsets(st.stream, reinterpret_cast<unsigned long long *>(cp.indptr.p), nv);
                // the one value that comes back: the device's lengths add up to the plan's
                const uint64_t got = SCANRS_D2H_VALUE(cp.indptr.p + nv, st.stream);
                if (got != nnz)
                    fail(SCANRS_ERR_DEVICE, "internal: the lengths of an export slab (%llu entries) do not match the plan (%llu)", (unsigned long long)got, (unsigned long long)nnz);
                launch_export_start(st.stream, from, g0, nv, cp.indptr.p, d_start.p);
                launch_export_pull(st.stream, from, g0, cp.indptr.p, d_start.p, nv, nnz, outer_global, cp.indices.p, cp.values.p);
                SCANRS_SYNC(st.stream); // the start table is released on return
            });
        });

    // encode: the slab as any SparseCopy; the arenas come down into the export's own memory, then the slab goes
    if (rc == SCANRS_OK)
        rc = fan_out(mm, [&](size_t d) {
            return guard([&] {
                Storage &st = *mm->shards[d]->st;
                CurrentHandle cur(&st);
                PhaseClock clock(st.export_us[2]);
                adaptive_export_encode(e.get(), (uint32_t)d, st, slab[d], force_kind, slab_bounds[d], &arena_bytes[d]);
                slab[d] = SparseCopy();
                device_free_flush(); // the stream is idle here
            });
        });

    // whatever is left of the slabs goes back under the handle that made it (a failure; nothing after a success)
    const auto drop_slabs = [&] {
        for (uint32_t d = 0; d < n; d++) {
            if (!slab[d].indptr.p && !slab[d].indices.p && !slab[d].values.p) continue;
            (void)hipSetDevice(mm->devices[d]);
            CurrentHandle cur(mm->shards[d]->st.get(), true);
            slab[d] = SparseCopy();
            device_free_flush();
        }
    };
    if (rc == SCANRS_OK) rc = guard([&] { adaptive_export_finish(e.get(), slab_bounds, moved, arena_bytes); });
    if (rc != SCANRS_OK) return failed(rc, drop_slabs);
    *out = e.release();
    return SCANRS_OK;
}

} // namespace

extern "C" {

int scanrs_multi_to_adaptive(scanrs_multi *mm, int major, int force_kind, scanrs_adaptive_export **out) {
    // everything that can be refused is refused here, before any device work
    if (const int rc = guard([&] { adaptive_check_export_args(mm, major, force_kind, out); })) return rc;
    return multi_to_adaptive(mm, major, force_kind, out);
}

} // extern "C"
