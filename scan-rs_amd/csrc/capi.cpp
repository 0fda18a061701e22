// The operator layer (the sqz::AdaptiveMat / LowRankOffset / scan-rs::normalization surface: creation, map and offset, products,
// normalisation, select) and its extern "C" boundary, with the options and counters; the sSeq and merge_clusters entry points sit
// next to their host logic. See include/scanrs_amd.h for the reference citations per entry point.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "col_moments_plan.hpp"
#include "bk_plan.hpp"
#include "knn_metric.hpp"
#include "spmm_route.hpp"
#include "transpose_plan.hpp"
#include "shard_exchange.hpp"

namespace scanrs {

// One exchange step. With the library's own transport (scanrs_mat_set_shard_comm) the collective is enqueued on the
// handle's stream; the host hook form synchronises first (the hook's runtime knows nothing of our stream).
static void allreduce_any(Storage &st, void *d, uint64_t count, int dtype) {
    if (!st.shard.active()) return;
    if (st.prof.on) st.prof.begin(st.stream, dtype == 0 ? "allreduce_f64" : "allreduce_u64", (double)count * 8.0);
    if (st.shard.comm) {
        comm_allreduce(st, st.shard.comm, d, count, dtype);
    } else if (st.shard.allreduce) {
        SCANRS_SYNC(st.stream);
        if (st.shard.allreduce(st.shard.ctx, d, count, dtype) != 0) fail(SCANRS_ERR_DEVICE, "all-reduce callback failed");
    } else {
        fail(SCANRS_ERR_ARGUMENT, "sharded handle without a transport");
    }
    if (st.prof.on) st.prof.end(st.stream);
}
void allreduce_f64(Storage &st, double *d, uint64_t count) { allreduce_any(st, d, count, 0); }
void allreduce_u64(Storage &st, unsigned long long *d, uint64_t count) { allreduce_any(st, d, count, 1); }
std::vector<unsigned long long> ShardExchange::gather_from(const unsigned long long *mine, uint64_t per_rank, bool on_host) {
    const hipStream_t s = st.stream;
    std::vector<unsigned long long> all((active() ? st.shard.world : 1) * per_rank);
    if (!active()) {
        if (on_host) {
            std::copy(mine, mine + per_rank, all.begin());
        } else {
            SCANRS_D2H(all.data(), mine, per_rank * 8, s);
            SCANRS_SYNC(s);
        }
        return all;
    }
    unsigned long long *d_all = st.scratch.get<unsigned long long>("shard_gather", all.size());
    unsigned long long *d_slot = d_all + st.shard.rank * per_rank;
    SCANRS_HIP(hipMemsetAsync(d_all, 0, all.size() * 8, s));
    if (on_host) {
        h2d(d_slot, mine, per_rank, s);
        SCANRS_SYNC(s); // `mine` may be pageable: it has been read before a step that fails can unwind the frame that holds it
    } else {
        SCANRS_HIP(hipMemcpyAsync(d_slot, mine, per_rank * 8, hipMemcpyDeviceToDevice, s));
    }
    sum(d_all, all.size());
    SCANRS_D2H(all.data(), d_all, all.size() * 8, s);
    SCANRS_SYNC(s);
    return all;
}
// primary's outer dimension is the sharded one: base rows when CSR, base cols when CSC
static bool base_rows_sharded(const Storage &st) { return st.shard.active() && st.storage == SCANRS_CSR; }
static bool base_cols_sharded(const Storage &st) { return st.shard.active() && st.storage == SCANRS_CSC; }
bool rows_sharded(const scanrs_mat *m) { return m->transposed ? base_cols_sharded(*m->st) : base_rows_sharded(*m->st); }
bool cols_sharded(const scanrs_mat *m) { return m->transposed ? base_rows_sharded(*m->st) : base_cols_sharded(*m->st); }

} // namespace scanrs

using namespace scanrs;

// ---- map translation ---------------------------------------------------------------------------------
DevMap scanrs_mat::dev_map(bool outer_is_view_row) const {
    DevMap dm;
    memset(&dm, 0, sizeof(dm));
    int n = 0;
    for (const auto &op : ops) {
        if (op.kind == OP_INTO) continue;
        if (n >= MAX_OPS) fail(SCANRS_ERR_ARGUMENT, "map chain longer than %d links", MAX_OPS);
        DevOp &d = dm.ops[n++];
        d.kind = op.kind;
        d.id = op.id;
        d.a = op.a ? op.a->p : nullptr;
        d.b = op.b ? op.b->p : nullptr;
        if (op.kind == OP_SCALE_AXIS) {
            // ScaleAxis wants r_op (axis 0) or c_op (axis 1); (r_op, c_op) = swap ? (c_v, r_v) : (r_v, c_v)
            const bool wants_view_row = (op.axis == 0) != op.swap;
            d.a_outer = wants_view_row == outer_is_view_row ? 1 : 0;
        } else if (op.kind == OP_BINOM_DEV || op.kind == OP_BINOM_PEARSON) {
            // a = n[c_op], b = pi[r_op]
            const bool a_wants_view_row = op.swap;
            d.a_outer = a_wants_view_row == outer_is_view_row ? 1 : 0;
            d.b_outer = 1 - d.a_outer;
        }
    }
    dm.n = n;
    return dm;
}

namespace scanrs {

// the copy whose outer dimension is the view's rows (true) or cols (false)
static SparseCopy &copy_outer_view_rows(scanrs_mat *m, bool view_rows) {
    return m->st->copy_with_outer_rows(view_rows != m->transposed);
}

// A solver alternates V x and V^T y. What the SECOND product of its first iteration needs — the transposed copy when it does not
// exist yet, and that orientation's tile layout when the auto path will take it — is built by a helper thread on a stream of its
// own while the main thread builds the first product's layout and runs the first pass (the only call Cell Ranger ever makes is the
// first one on a fresh handle, tools/src/bin/cmd.rs:61-70: serially these builds were more than half of it). The helper touches
// nothing but the copy it builds; whoever needs that copy joins the helper first (side_join_if).
// normalize() starts it already (solver_follows): the one thing a caller does with a scaled and centred matrix is a PCA, and the
// helper then also runs beside the normalisation passes ("side_build" 0: nothing is built before a product asks for it).
void prepare_second_orientation(scanrs_mat *m, bool transpose_second, bool solver_follows) {
    Storage &st = *m->st;
    if (st.side || !st.opt.side_build) return;
    if (st.primary.nnz < (1ull << 22)) return; // small matrices: the builds take less than starting a thread
    const bool second_outer_rows = (!transpose_second) != m->transposed; // the base-matrix dimension the second product's outer vectors run over
    const bool second_is_primary = second_outer_rows == (st.storage == SCANRS_CSR);
    SparseCopy *second = second_is_primary ? &st.primary : &st.other, *first = second_is_primary ? &st.other : &st.primary;
    // Against tiles_static_candidate, the launch's own test:
    //  - the auto path only: a forced path 3 builds its layout inside the product, whatever the overflow, and the helper's
    //    tile_layout_build_auto would apply the overflow limit to it;
    //  - a solver is running or follows (this site's own term: one product alone builds nothing ahead);
    //  - the size of `primary` stands for both copies (the transposed one may not exist yet; the nonzeros are the same);
    //  - no tile_shape_ok and no tile_visits_fit: the helper's tile_layout_build_auto tests both before it builds anything;
    //  - no panel terms: the widths are the solver's.
    const Options &o = st.opt;
    const bool tiles_wanted = path_auto(o) && o.tile_auto && f64_panels(o) && (st.tile_hint > 0 || solver_follows) && tile_auto_size(o, st.primary.nnz);
    auto exists = [&](const SparseCopy *c) { return c == &st.primary || st.has_other; };
    // the first product's layout too (the helper builds it FIRST, alone on the device, while the caller normalizes; the transposition
    // then runs beside the first pass, which is bound by the vector pipe, not by memory) — but only from normalize on: inside a solver
    // the caller is about to build it himself
    const bool first_layout = tiles_wanted && solver_follows && first->tiles == nullptr;
    const bool second_layout = tiles_wanted && second->tiles == nullptr;
    const bool need_second_copy = !exists(second);
    if (!first_layout && !second_layout && !need_second_copy) return;
    int dev = 0;
    SCANRS_HIP(hipGetDevice(&dev));
    auto *sb = new Storage::SideBuild();
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (hipStreamCreateWithPriority(&sb->stream, hipStreamNonBlocking, least) != hipSuccess) {
        (void)hipGetLastError();
        delete sb;
        return; // no helper: the main thread builds on demand as before
    }
    int n = 0;
    if (first_layout) {
        sb->order[n] = first;
        sb->want_layout[n] = true;
        n++;
    }
    sb->order[n] = second;
    sb->want_layout[n] = second_layout;
    registry_set_side(st, sb);
    Storage *stp = &st;
    sb->th = std::thread([stp, sb, dev] {
        const auto t0 = std::chrono::steady_clock::now();
        auto mark = [&](int pos, bool layout) {
            std::lock_guard<std::mutex> lk(sb->mu);
            (layout ? sb->layout_done : sb->copy_done)[pos] = true;
            sb->cv.notify_all();
        };
        try {
            SCANRS_HIP(hipSetDevice(dev));
            CurrentHandle cur(stp);
            for (int pos = 0; pos < 2; pos++) {
                SparseCopy *cp = const_cast<SparseCopy *>(sb->order[pos]);
                if (!cp) continue;
                if (cp == &stp->other && !stp->has_other) {
                    build_transposed_copy(*stp, stp->primary, stp->other, sb->stream);
                    stp->has_other = true;
                }
                mark(pos, false);
                if (sb->want_layout[pos]) {
                    (void)tile_layout_build_auto(*stp, *cp, sb->stream);
                    wait_stream(sb->stream, "side build", __FILE__, __LINE__);
                }
                mark(pos, true);
            }
        } catch (const Failure &e) {
            std::lock_guard<std::mutex> lk(sb->mu);
            sb->code = e.code;
            sb->err = scanrs_last_error(); // this thread's message buffer
        } catch (const std::exception &e) {
            std::lock_guard<std::mutex> lk(sb->mu);
            sb->code = SCANRS_ERR_DEVICE;
            sb->err = std::string("side build: ") + e.what();
        }
        sb->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::lock_guard<std::mutex> lk(sb->mu);
        sb->finished = true;
        sb->cv.notify_all();
    });
}

void mat_apply(scanrs_mat *m, bool transpose, const double *dX, uint32_t ldx, uint32_t l, double *dOut, uint32_t ldo) {
    Storage &st = *m->st;
    CurrentHandle cur(&st);
    const bool outer_is_view_row = !transpose;
    SparseCopy &cp = copy_outer_view_rows(m, outer_is_view_row);
    st.side_join_if(&cp, true); // its tile layout may be in the making
    DevMap map = m->dev_map(outer_is_view_row);
    const double *off_a = nullptr, *off_w = nullptr;
    // A map that ENDS in a ScaleAxis indexed by the inner position — the per-gene 1/sigma when cells are the outer
    // vectors — is linear in the gathered row: out[o,:] = sum_i f(v,o,i) a[i] X[i,:] = sum_i f(v,o,i) (a[i] X[i,:]).
    // Scaling the panel once (n_inner x l) replaces one scattered 8-byte gather per nonzero per pass (-2.4 ms of a 43 ms pass).
    const double *dXs = dX;
    while (map.n > 0 && map.ops[map.n - 1].kind == OP_SCALE_AXIS && !map.ops[map.n - 1].a_outer && l > 0 && cp.n_inner > 0) {
        const bool again = dXs != dX;
        double *xs = st.scratch.get<double>(again ? "map_xs2" : "map_xs", (size_t)cp.n_inner * ldx);
        launch_scale_rows(st, dXs, ldx, cp.n_inner, l, map.ops[map.n - 1].a, xs);
        dXs = xs;
        map.n--;
    }
    uint32_t ldw = 0;
    if (m->off_rank) {
        // A R = mat R + u (v R);  A^T Y = mat^T Y + v^T (u^T Y)   (sqz/src/low_rank_offset.rs:76-95)
        const double *B = transpose ? m->off_u->p : m->off_v->p; // n_in x rank
        off_a = transpose ? m->off_v->p : m->off_u->p;           // n_out x rank
        ldw = even_up(l);
        double *w = st.scratch.get<double>("off_w", (size_t)m->off_rank * ldw);
        // the dense tile product stages a compact copy of the panel: written here, from the read the column sums make anyway
        double *xc = dXs == dX ? tile_panel_copy_target(st, cp, l) : nullptr;
        launch_weighted_colsum(st, B, m->off_rank, dX, ldx, cp.n_inner, l, w, ldw, xc, l);
        if (xc) {
            st.tile_xc_src = dX;
            st.tile_xc_l = l;
        }
        off_w = w;
    }
    launch_spmm_f64(st, cp, map, dXs, ldx, l, dOut, ldo, off_a, m->off_rank, off_w, ldw);
    st.tile_xc_src = nullptr;
    // contraction over the sharded dimension -> partial sums on every rank
    const bool contraction_sharded = transpose ? rows_sharded(m) : cols_sharded(m);
    if (contraction_sharded) allreduce_f64(st, dOut, (uint64_t)cp.n_outer * ldo);
}

static std::shared_ptr<DevBuf<double>> upload_vec(Storage &st, const double *h, size_t n) {
    auto b = std::make_shared<DevBuf<double>>(std::max<size_t>(n, 1));
    if (n) SCANRS_HIP(hipMemcpyAsync(b->p, h, n * 8, hipMemcpyHostToDevice, st.stream));
    SCANRS_SYNC(st.stream);
    return b;
}

std::shared_ptr<Storage> new_storage(uint64_t rows, uint64_t cols, int storage) {
    auto st = std::make_shared<Storage>();
    registry_add(st.get());
    st->rows = rows;
    st->cols = cols;
    st->storage = storage;
    // a blocking stream: legacy null-stream copies (ours and the host program's, e.g. torch's default
    // stream that produced a device-resident input) stay ordered with the kernels launched here
    SCANRS_HIP(hipStreamCreate(&st->stream));
    st->scratch.stream = st->stream;
    return st;
}

static void create_common(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices,
                          const uint32_t *values, bool device_src, scanrs_mat **out, bool sort_first = false) {
    Tick tick("create: upload + validate");
    if (!out) fail(SCANRS_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    need_device();
    jump_tables_prefetch(); // the GF(2) tables of the seeded start panel (solver.cpp): ~10 ms of one host core, off the first PCA's path
    if (storage != SCANRS_CSR && storage != SCANRS_CSC) fail(SCANRS_ERR_ARGUMENT, "storage must be 0 (CSR) or 1 (CSC)");
    if (!indptr) fail(SCANRS_ERR_ARGUMENT, "null indptr");
    if (rows > 0xFFFFFFFFull || cols > 0xFFFFFFFFull) fail(SCANRS_ERR_SHAPE, "dimensions must fit in u32 (AdaptiveVec limit)");
    auto st = new_storage(rows, cols, storage);
    SparseCopy &cp = st->primary;
    cp.n_outer = storage == SCANRS_CSR ? rows : cols;
    cp.n_inner = storage == SCANRS_CSR ? cols : rows;
    const hipMemcpyKind kind = device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    CurrentHandle cur(st.get());
    auto lap = [&, t_prev = std::chrono::steady_clock::now()](const char *what) mutable { // SCANRS_TRACE=1: the phases of a creation (each forces a sync)
        if (!trace_on()) return;
        (void)wait_stream_quiet(st->stream);
        const auto t_now = std::chrono::steady_clock::now();
        fprintf(stderr, "[scanrs trace]   create: %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t_now - t_prev).count());
        t_prev = t_now;
    };
    cp.indptr.alloc(cp.n_outer + 1);
    // a device-resident input was produced on the caller's streams: the blocking stream of the handle is ordered behind the legacy
    // null stream (torch's default stream), anything else is the caller's to synchronise before the call
    SCANRS_HIP(hipMemcpyAsync(cp.indptr.p, indptr, (cp.n_outer + 1) * 8, kind, st->stream));
    uint64_t first = 0, last = 0;
    first = SCANRS_D2H_VALUE(cp.indptr.p, st->stream);
    last = SCANRS_D2H_VALUE(cp.indptr.p + cp.n_outer, st->stream);
    SCANRS_SYNC(st->stream);
    if (first != 0) fail(SCANRS_ERR_ARGUMENT, "indptr[0] must be 0");
    cp.nnz = last;
    if (cp.nnz && (!indices || !values)) fail(SCANRS_ERR_ARGUMENT, "null indices/values");
    cp.indices.alloc(std::max<uint64_t>(1, cp.nnz));
    cp.values.alloc(std::max<uint64_t>(1, cp.nnz));
    if (cp.nnz) {
        SCANRS_HIP(hipMemcpyAsync(cp.indices.p, indices, cp.nnz * 4, kind, st->stream));
        SCANRS_HIP(hipMemcpyAsync(cp.values.p, values, cp.nnz * 4, kind, st->stream));
        if (!device_src) SCANRS_SYNC(st->stream); // the caller's host arrays may be pageable and are his again on return
    }
    lap("copies");
    if (sort_first) sort_outer_vectors(*st, cp);
    uint64_t zeros = 0, bad = 0;
    validate_copy(*st, cp, &zeros, &bad);
    lap("validation");
    if (bad) fail(SCANRS_ERR_ARGUMENT, "indices must be in range and strictly ascending within each outer vector (%llu violations)", (unsigned long long)bad);
    if (zeros) compact_nonzeros(*st, cp);
    cp.build_items(st->stream);
    lap("work items");
    device_free_flush(); // the stream is idle here
    auto *m = new scanrs_mat();
    m->st = st;
    *out = m;
}

// A handle around a copy that was made on the device (select / partition): its buffers are adopted, not copied, and nothing goes
// through the host. The copy comes from the library's own kernels (indices in range and ascending, no zeros), so the validation of
// scanrs_mat_create_device has nothing to find; everything else is as create_common leaves it.
static scanrs_mat *adopt_copy(uint64_t rows, uint64_t cols, int storage, SparseCopy &&made) {
    auto st = new_storage(rows, cols, storage);
    SparseCopy &cp = st->primary;
    cp.n_outer = made.n_outer;
    cp.n_inner = made.n_inner;
    cp.nnz = made.nnz;
    cp.max_value = made.nnz ? std::max(made.max_value, 1u) : 0u;
    cp.indptr = std::move(made.indptr);
    cp.indices = std::move(made.indices);
    cp.values = std::move(made.values);
    if ((storage == SCANRS_CSR ? rows : cols) != cp.n_outer || (storage == SCANRS_CSR ? cols : rows) != cp.n_inner)
        fail(SCANRS_ERR_SHAPE, "internal: adopted copy does not match the handle's shape");
    CurrentHandle cur(st.get());
    cp.build_items(st->stream);
    auto *m = new scanrs_mat();
    m->st = st;
    return m;
}

// select / partition work on the stored counts under the identity map (the reference clones the map verbatim and would index its
// per-axis vectors with the NEW positions; that is not reproduced)
static void need_plain(const scanrs_mat *m, const char *what) {
    if (!map_is_raw(m))
        fail(SCANRS_ERR_ARGUMENT, "%s: the handle's map is not the identity (a scaling or a function has been composed); call scanrs_mat_reset_map first", what);
    if (m->off_rank) fail(SCANRS_ERR_ARGUMENT, "%s: the handle has a low-rank offset (center / scale_and_center / normalize); call scanrs_mat_reset_map first", what);
}
// the plain entry points are not collective calls: a sharded handle goes through the *_sharded ones (collective: true)
static void need_plain_unsharded(const scanrs_mat *m, const char *what, bool collective = false) {
    need_plain(m, what);
    if (!collective && m->st->shard.active())
        fail(SCANRS_ERR_ARGUMENT, "%s of a sharded handle (scanrs_mat_set_shard*) is not supported; the collective scanrs_mat_%s_sharded serves one", what, what);
}

// a result of a collective select / partition: rank r of the same world on the same transport as its source, over its own range
static void bind_like(const Storage &src, scanrs_mat *result, uint64_t outer_begin, uint64_t outer_global) {
    ShardInfo &sh = result->st->shard;
    sh = src.shard;
    sh.outer_begin = outer_begin;
    sh.outer_global = outer_global;
}
// rows / cols of the handle that adopts a copy made under the storage flag `view_storage`
static uint64_t made_rows(const SparseCopy &c, int view_storage) { return view_storage == SCANRS_CSR ? c.n_outer : c.n_inner; }
static uint64_t made_cols(const SparseCopy &c, int view_storage) { return view_storage == SCANRS_CSR ? c.n_inner : c.n_outer; }

static void select_axis(scanrs_mat *m, bool rows_axis, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out, bool collective = false) {
    if (!m || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
    *out = nullptr;
    need_device();
    need_plain_unsharded(m, rows_axis ? "select_rows" : "select_cols", collective);
    Storage &st = *m->st;
    const bool outer_is_view_rows = (st.storage == SCANRS_CSR) != m->transposed;
    const int view_storage = m->transposed ? 1 - st.storage : st.storage;
    const bool sharded = st.shard.active();
    uint64_t out_begin = st.shard.outer_begin, out_global = st.shard.outer_global; // a list along the replicated dimension leaves the ranges alone
    SparseCopy made;
    {
        CurrentHandle cur(&st);
        if (rows_axis != outer_is_view_rows) {
            select_inner(st, st.primary, idx, n_idx, made);
        } else if (sharded) {
            select_outer_sharded(st, st.primary, idx, n_idx, made, &out_begin);
            out_global = n_idx;
        } else {
            select_outer(st, st.primary, idx, n_idx, made);
        }
        device_free_flush();
    }
    scanrs_mat *h = adopt_copy(made_rows(made, view_storage), made_cols(made, view_storage), view_storage, std::move(made));
    if (sharded) bind_like(st, h, out_begin, out_global);
    *out = h;
}

// radix select of the k-th smallest (0-based, global rank) of a u32 device array spread over ranks
static uint32_t select_kth(Storage &st, const uint32_t *d, uint64_t n_local, uint64_t kth) {
    unsigned long long *hist = st.scratch.get<unsigned long long>("select_hist", 4096);
    std::vector<unsigned long long> h(4096);
    uint32_t prefix = 0, mask = 0;
    const uint32_t shifts[3] = {20, 8, 0};
    const uint32_t bits[3] = {12, 12, 8};
    for (int pass = 0; pass < 3; pass++) {
        launch_hist12(st, d, n_local, shifts[pass], (1u << bits[pass]) - 1u, mask, prefix, hist);
        allreduce_u64(st, hist, 4096);
        SCANRS_D2H(h.data(), hist, 4096 * 8, st.stream);
        const uint32_t nb = 1u << bits[pass];
        uint32_t bin = 0;
        for (; bin < nb; bin++) {
            if (kth < h[bin]) break;
            kth -= h[bin];
        }
        if (bin == nb) fail(SCANRS_ERR_NUMERICAL, "median selection ran past the histogram");
        prefix |= bin << shifts[pass];
        mask |= (nb - 1u) << shifts[pass];
    }
    return prefix;
}

// median_mut (scan-rs/src/stats.rs:13-38) of a distributed u32 array; n = global count
static bool median_u32(Storage &st, const uint32_t *d, uint64_t n_local, uint64_t n_global, uint32_t *out) {
    if (n_global == 0) return false;
    if (n_global % 2 == 0) {
        const uint32_t hi = select_kth(st, d, n_local, n_global / 2);
        const uint32_t lo = select_kth(st, d, n_local, n_global / 2 - 1);
        *out = (uint32_t)(hi + lo) / 2u; // integer midpoint in T = u32 (wrapping add as rustc release)
    } else {
        *out = select_kth(st, d, n_local, n_global / 2);
    }
    return true;
}

static void log_normalize_impl(scanrs_mat *m, double umi_count_sum, int log_fn, const uint32_t *size_factors) {
    // log_normalize_with_size_factor, scan-rs/src/normalization.rs:138-178
    Tick tk("normalize: log_normalize");
    if (!map_is_raw(m) || m->off_rank) fail(SCANRS_ERR_ARGUMENT, "log_normalize needs the raw count matrix (AdaptiveMat<u32>)");
    if (log_fn != OP_LN_1P && log_fn != OP_LOG2_1P && log_fn != OP_LOG10_1P) fail(SCANRS_ERR_ARGUMENT, "bad log base");
    if (rows_sharded(m)) fail(SCANRS_ERR_ARGUMENT, "normalisation needs the barcode (column) dimension to be the sharded one");
    Storage &st = *m->st;
    const uint64_t ncols = m->cols();
    CurrentHandle cur(&st);
    SparseCopy &cp = copy_outer_view_rows(m, false); // outer = view cols (barcodes)
    DevMap raw;
    memset(&raw, 0, sizeof(raw));
    uint32_t *counts = st.scratch.get<uint32_t>("norm_counts", std::max<uint64_t>(1, ncols));
    launch_row_reduce(st, cp, raw, 0, counts, nullptr, nullptr); // matrix.sum_axis(Axis(0)) :159,161
    double target;
    if (umi_count_sum >= 0.0) {
        target = umi_count_sum;
    } else {
        const uint64_t n_global = cols_sharded(m) ? st.shard.outer_global : ncols;
        uint32_t med = 0;
        target = median_u32(st, counts, ncols, n_global, &med) ? std::max((double)med, 1.0) : 1.0; // :162-168
    }
    m->target_umi = target;
    const uint32_t *norm_counts = counts;
    if (size_factors) {
        uint32_t *sf = st.scratch.get<uint32_t>("norm_sf", std::max<uint64_t>(1, ncols));
        if (ncols) SCANRS_HIP(hipMemcpyAsync(sf, size_factors, ncols * 4, hipMemcpyHostToDevice, st.stream));
        SCANRS_SYNC(st.stream);
        norm_counts = sf;
    }
    auto scales = std::make_shared<DevBuf<double>>(std::max<uint64_t>(1, ncols));
    launch_u32_to_scale(st, norm_counts, ncols, target, scales->p); // col_scales :169
    MapOp sc;
    sc.kind = OP_SCALE_AXIS;
    sc.axis = 1;
    sc.a = scales;
    m->ops.push_back(sc); // compose_map(scale_cols)
    MapOp lg;
    lg.kind = log_fn;
    m->ops.push_back(lg); // .apply(log1p_fn) :177
    SCANRS_SYNC(st.stream);
}

// per-`axis` sums of mapped values: axis 1 -> per view row, axis 0 -> per view col; reduced across ranks
// when the summed-over dimension is sharded.
static void axis_sums(scanrs_mat *m, int axis, int mode, double *d_sum, double *d_sumsq) {
    Storage &st = *m->st;
    CurrentHandle cur(&st);
    const bool outer_view_rows = axis == 1;
    // From the copy whose outer vectors are the SUMMED-OVER axis when the map allows it (normalize_ops.hip, col_moments_kernel: a
    // per-outer table instead of one logarithm per nonzero) and that copy exists already; else the ordinary pass over the copy
    // whose outer vectors are the slices.
    bool done = false;
    if (st.opt.col_moments && mode != 0) {
        const bool other_outer_rows = (!outer_view_rows) != m->transposed;
        // (other_settled, not has_other: whether the helper thread has finished the transposed copy by now depends on its speed, and the
        // two passes round differently: the moments - and the PCA behind them - must not change from run to run)
        const bool exists = other_outer_rows == (st.storage == SCANRS_CSR) || st.other_settled;
        if (exists) {
            SparseCopy &co = copy_outer_view_rows(m, !outer_view_rows);
            if (st.opt.col_moments == 2 || co.nnz >= st.opt.blocked_min_nnz) done = launch_col_moments(st, co, m->dev_map(!outer_view_rows), mode, d_sum, d_sumsq);
        }
    }
    SparseCopy &cp = done ? copy_outer_view_rows(m, !outer_view_rows) : copy_outer_view_rows(m, outer_view_rows);
    if (!done) {
        const DevMap map = m->dev_map(outer_view_rows);
        launch_row_reduce(st, cp, map, mode, nullptr, d_sum, d_sumsq);
    }
    const uint64_t n_out = done ? cp.n_inner : cp.n_outer;
    const bool contraction_sharded = outer_view_rows ? cols_sharded(m) : rows_sharded(m);
    if (contraction_sharded) {
        allreduce_f64(st, d_sum, n_out);
        if (mode == 2) allreduce_f64(st, d_sumsq, n_out);
    }
}
// shape()[axis] as the reference's mean_axis divides by (sqz/src/mat.rs:274), global when sharded
static double axis_extent(const scanrs_mat *m, int axis) {
    const bool sharded = axis == 0 ? rows_sharded(m) : cols_sharded(m);
    if (sharded) return (double)m->st->shard.outer_global;
    return (double)(axis == 0 ? m->rows() : m->cols());
}

static void set_offset_dev(scanrs_mat *m, uint32_t rank, std::shared_ptr<DevBuf<double>> u_rows_by_rank,
                           std::shared_ptr<DevBuf<double>> v_cols_by_rank) {
    m->off_rank = rank;
    m->off_u = std::move(u_rows_by_rank);
    m->off_v = std::move(v_cols_by_rank);
}

static void scale_and_center_impl(scanrs_mat *m, int axis, const double *given_scaling) {
    // sqz/src/mat.rs:986-1001
    Tick tk("normalize: scale_and_center");
    stage_mark("scale_and_center");
    if (axis != 0 && axis != 1) fail(SCANRS_ERR_ARGUMENT, "axis must be 0 or 1");
    if (m->off_rank) fail(SCANRS_ERR_ARGUMENT, "matrix already carries a low-rank offset");
    Storage &st = *m->st;
    const uint64_t n = axis == 1 ? m->rows() : m->cols();     // number of slices
    CurrentHandle cur(&st);
    const uint64_t other = axis == 1 ? m->cols() : m->rows(); // local length of each slice
    double *sum = st.scratch.get<double>("mom_sum", std::max<uint64_t>(1, n));
    double *sumsq = st.scratch.get<double>("mom_sumsq", std::max<uint64_t>(1, n));
    axis_sums(m, axis, given_scaling ? 1 : 2, sum, sumsq);
    double *scale_in = nullptr;
    if (given_scaling) {
        scale_in = st.scratch.get<double>("mom_scale_in", std::max<uint64_t>(1, n));
        if (n) SCANRS_HIP(hipMemcpyAsync(scale_in, given_scaling, n * 8, hipMemcpyHostToDevice, st.stream));
        SCANRS_SYNC(st.stream);
    }
    auto neg = std::make_shared<DevBuf<double>>(std::max<uint64_t>(1, n));
    auto inv = std::make_shared<DevBuf<double>>(std::max<uint64_t>(1, n));
    launch_finish_moments(st, sum, sumsq, n, axis_extent(m, axis), given_scaling ? 1 : 0, scale_in, neg->p, inv->p, nullptr);
    MapOp sc; // scale(axis, Some(s)): ScaleAxis(Axis(1 - axis), 1/s)
    sc.kind = OP_SCALE_AXIS;
    sc.axis = 1 - axis;
    sc.a = inv;
    m->ops.push_back(sc);
    auto ones = std::make_shared<DevBuf<double>>(std::max<uint64_t>(1, other));
    launch_fill_f64(st, ones->p, other, 1.0);
    // center(axis, Some(means)): axis 1 -> u = -means (rows x 1), v = 1; axis 0 -> u = 1, v = -means
    if (axis == 1)
        set_offset_dev(m, 1, neg, ones);
    else
        set_offset_dev(m, 1, ones, neg);
    SCANRS_SYNC(st.stream);
}

static void binom_impl(scanrs_mat *m, int kind) {
    // binom_deviance_resid / binom_pearson_resid, scan-rs/src/normalization.rs:232-322
    if (!map_is_raw(m) || m->off_rank) fail(SCANRS_ERR_ARGUMENT, "binomial residuals need the raw count matrix");
    if (rows_sharded(m)) fail(SCANRS_ERR_ARGUMENT, "normalisation needs the barcode (column) dimension to be the sharded one");
    Storage &st = *m->st;
    const uint64_t R = m->rows(), C = m->cols();
    auto n = std::make_shared<DevBuf<double>>(std::max<uint64_t>(1, C));
    auto pi = std::make_shared<DevBuf<double>>(std::max<uint64_t>(1, R));
    auto u = std::make_shared<DevBuf<double>>(std::max<uint64_t>(1, R));
    auto v = std::make_shared<DevBuf<double>>(std::max<uint64_t>(1, C));
    double *rowsum = st.scratch.get<double>("binom_rowsum", std::max<uint64_t>(1, R));
    double *tot = st.scratch.get<double>("binom_total", 1);
    axis_sums(m, 0, 1, n->p, nullptr);  // n = sum_axis::<f64>(Axis(0))
    axis_sums(m, 1, 1, rowsum, nullptr); // sum_axis::<f64>(Axis(1))
    launch_sum_f64(st, n->p, C, tot);
    if (cols_sharded(m)) allreduce_f64(st, tot, 1);
    const double total = SCANRS_D2H_VALUE(tot, st.stream);
    launch_binom_uv(st, kind, n->p, C, rowsum, R, total, pi->p, u->p, v->p);
    MapOp op;
    op.kind = kind;
    op.a = n;
    op.b = pi;
    m->ops.clear();
    m->ops.push_back(op); // matrix.set_map(dev_resid_map)
    set_offset_dev(m, 1, u, v);
    SCANRS_SYNC(st.stream);
}

// Upload of an n_in x l panel (`in_is_l_by_n`: given as l x n_in, transposed on the way), `product(dX, ld, dY)`, download of the
// n_out x l result (transposed back likewise). The caller has made the handle current.
template <typename T, typename Product>
static void dot_through_scratch(scanrs_mat *m, bool transpose, const T *h_in, uint32_t l, T *h_out, bool in_is_l_by_n, const char *key_in,
                                const char *key_out, Product &&product) {
    Storage &st = *m->st;
    const uint64_t n_in = transpose ? m->rows() : m->cols();
    const uint64_t n_out = transpose ? m->cols() : m->rows();
    if (l == 0) return;
    const uint32_t ld = even_up(l);
    T *dX = st.scratch.get<T>(key_in, std::max<uint64_t>(1, n_in) * ld);
    T *dY = st.scratch.get<T>(key_out, std::max<uint64_t>(1, n_out) * ld);
    SCANRS_HIP(hipMemsetAsync(dX, 0, std::max<uint64_t>(1, n_in) * ld * sizeof(T), st.stream));
    std::vector<T> tmp;
    const T *src = h_in;
    if (in_is_l_by_n) {
        tmp.resize((size_t)n_in * l);
        for (uint32_t i = 0; i < l; i++)
            for (uint64_t j = 0; j < n_in; j++) tmp[j * l + i] = h_in[(size_t)i * n_in + j];
        src = tmp.data();
    }
    if (n_in)
        SCANRS_HIP(hipMemcpy2DAsync(dX, (size_t)ld * sizeof(T), src, (size_t)l * sizeof(T), (size_t)l * sizeof(T), n_in, hipMemcpyHostToDevice, st.stream));
    SCANRS_SYNC(st.stream);
    product(dX, ld, dY);
    std::vector<T> res((size_t)n_out * l);
    SCANRS_D2H_2D(res.data(), dY, (size_t)ld * sizeof(T), (size_t)l * sizeof(T), n_out, st.stream);
    SCANRS_SYNC(st.stream);
    if (in_is_l_by_n) {
        for (uint64_t j = 0; j < n_out; j++)
            for (uint32_t i = 0; i < l; i++) h_out[(size_t)i * n_out + j] = res[j * l + i];
    } else if (!res.empty()) {
        memcpy(h_out, res.data(), res.size() * sizeof(T));
    }
}

} // namespace scanrs

// =================================================================================================
extern "C" {

int scanrs_device_available(void) {
    try {
        return device_ok() ? 1 : 0;
    } catch (...) {
        return 0;
    }
}
const char *scanrs_version(void) { return "scanrs_amd 0.1.0 (gfx950)"; }
int scanrs_init(void) {
    return guard([&] {
        need_device();
        jump_tables_prefetch();
        library_warm_up();
        try { // best effort: a host that cannot pin 72 MB now will find out (and say so) when a call needs the buffer
            size_t got = 0;
            void *p = pinned_take((size_t)72 << 20, &got); // the staging ring of a 10^6 x 50 delivery (67 MB) and the start panel
            pinned_give(p, got);
        } catch (const Failure &) {
            (void)hipGetLastError();
        }
    });
}
int scanrs_release_cached_memory(void) {
    return guard([&] { device_cache_release(); });
}
int scanrs_reserve_device_memory(uint64_t bytes) {
    return guard([&] {
        need_device();
        device_reserve((size_t)bytes);
    });
}
int scanrs_cached_memory_bytes(uint64_t *bytes) {
    return guard([&] {
        if (!bytes) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *bytes = device_cache_bytes();
    });
}
int scanrs_device_memory_in_use(uint64_t *bytes) {
    return guard([&] {
        if (!bytes) fail(SCANRS_ERR_ARGUMENT, "null argument");
        device_free_flush();
        *bytes = device_live_bytes();
        if (trace_on()) device_memory_report("scanrs_device_memory_in_use");
    });
}

int scanrs_mat_create(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices,
                      const uint32_t *values, scanrs_mat **out) {
    return guard([&] { create_common(rows, cols, storage, indptr, indices, values, false, out); });
}
int scanrs_mat_create_unsorted(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices,
                               const uint32_t *values, scanrs_mat **out) {
    return guard([&] { create_common(rows, cols, storage, indptr, indices, values, false, out, true); });
}
int scanrs_mat_create_device(uint64_t rows, uint64_t cols, int storage, const uint64_t *d_indptr, const uint32_t *d_indices,
                             const uint32_t *d_values, scanrs_mat **out) {
    return guard([&] { create_common(rows, cols, storage, d_indptr, d_indices, d_values, true, out); });
}
int scanrs_mat_create_adaptive(uint64_t rows, uint64_t cols, int storage, const scanrs_adaptive_vec *vecs, uint64_t n_vecs,
                               scanrs_mat **out) {
    return guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null output handle");
        *out = nullptr;
        need_device();
        if (storage != SCANRS_CSR && storage != SCANRS_CSC) fail(SCANRS_ERR_ARGUMENT, "storage must be 0 (CSR) or 1 (CSC)");
        const uint64_t n_outer = storage == SCANRS_CSR ? rows : cols, n_inner = storage == SCANRS_CSR ? cols : rows;
        if (n_vecs != n_outer) fail(SCANRS_ERR_SHAPE, "one AdaptiveVec per outer vector is required");
        if (n_vecs > 0 && !vecs) fail(SCANRS_ERR_ARGUMENT, "null vector table");
        DevBuf<uint64_t> ip;
        DevBuf<uint32_t> ix, vv;
        decode_adaptive_vectors(vecs, n_vecs, n_inner, ip, ix, vv);
        ::scanrs::wait_device(__PRETTY_FUNCTION__, __FILE__, __LINE__);
        create_common(rows, cols, storage, ip.p, ix.p, vv.p, true, out); // validates ordering, copies into the handle
    });
}
void scanrs_mat_free(scanrs_mat *m) {
    if (!m) return;
    const Storage *owner = m->st.get();
    const bool last = m->st.use_count() == 1;
    {
        DyingHandle dying(last ? owner : nullptr);
        CurrentHandle cur(last ? current_handle() : owner, true); // a view's own buffers (map arrays, offset): release events on the storage's streams, which live on
        delete m;
    }
    // the handle's buffers (when this was the last view of its storage): its streams were drained by the destructor, nobody else queued work on them
    if (last) device_free_flush_owner_gone(owner);
}

int scanrs_mat_view(const scanrs_mat *m, scanrs_mat **out) {
    return guard([&] {
        if (!m || !out) fail(SCANRS_ERR_ARGUMENT, "null handle");
        *out = new scanrs_mat(*m);
    });
}
int scanrs_mat_t(const scanrs_mat *m, scanrs_mat **out) {
    return guard([&] {
        if (!m || !out) fail(SCANRS_ERR_ARGUMENT, "null handle");
        auto *t = new scanrs_mat(*m);
        t->transposed = !m->transposed;
        for (auto &op : t->ops) op.swap = !op.swap; // TransposeMap (matrix_map.rs:42-80)
        std::swap(t->off_u, t->off_v);              // LowRankOffset::t (low_rank_offset.rs:60-65)
        *out = t;
    });
}
int scanrs_mat_shape(const scanrs_mat *m, uint64_t *rows, uint64_t *cols) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (rows) *rows = m->rows();
        if (cols) *cols = m->cols();
    });
}
int scanrs_mat_nnz(const scanrs_mat *m, uint64_t *nnz) {
    return guard([&] {
        if (!m || !nnz) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *nnz = m->st->primary.nnz;
    });
}
int scanrs_mat_storage(const scanrs_mat *m, int *storage) {
    return guard([&] {
        if (!m || !storage) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *storage = m->transposed ? 1 - m->st->storage : m->st->storage;
    });
}

int scanrs_mat_reset_map(scanrs_mat *m) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        CurrentHandle cur(m->st.get(), true); // the map's arrays and the offset go back with release events on this handle's streams (released outside any handle they were stranded)
        m->ops.clear();
        m->off_rank = 0;
        m->off_u.reset();
        m->off_v.reset();
    });
}
int scanrs_mat_compose_scale_axis(scanrs_mat *m, int axis, const double *factors) {
    return guard([&] {
        if (!m || !factors) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (axis != 0 && axis != 1) fail(SCANRS_ERR_ARGUMENT, "Only implemented for 2D arrays.");
        if (m->off_rank) fail(SCANRS_ERR_ARGUMENT, "cannot compose a map onto a LowRankOffset");
        MapOp op;
        op.kind = OP_SCALE_AXIS;
        op.axis = axis;
        op.a = upload_vec(*m->st, factors, axis == 0 ? m->rows() : m->cols());
        m->ops.push_back(op);
    });
}
int scanrs_mat_apply(scanrs_mat *m, int scalar_fn) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (scalar_fn < OP_LN_1P || scalar_fn > OP_SQUARE) fail(SCANRS_ERR_ARGUMENT, "unknown scalar map");
        if (m->off_rank) fail(SCANRS_ERR_ARGUMENT, "cannot compose a map onto a LowRankOffset");
        MapOp op;
        op.kind = scalar_fn;
        m->ops.push_back(op);
    });
}
int scanrs_mat_set_offset(scanrs_mat *m, uint32_t rank, const double *u, const double *v) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (rank == 0) {
            set_offset_dev(m, 0, nullptr, nullptr);
            return;
        }
        if (!u || !v) fail(SCANRS_ERR_ARGUMENT, "null offset factors");
        const uint64_t R = m->rows(), C = m->cols();
        std::vector<double> vt((size_t)C * rank); // v is rank x cols; keep cols x rank on the device
        for (uint32_t q = 0; q < rank; q++)
            for (uint64_t c = 0; c < C; c++) vt[c * rank + q] = v[(size_t)q * C + c];
        set_offset_dev(m, rank, upload_vec(*m->st, u, (size_t)R * rank), upload_vec(*m->st, vt.data(), vt.size()));
    });
}

static void host_axis_sums(scanrs_mat *m, int axis, int mode, std::vector<double> &s, std::vector<double> &s2) {
    if (axis != 0 && axis != 1) fail(SCANRS_ERR_ARGUMENT, "axis must be 0 or 1");
    Storage &st = *m->st;
    const uint64_t n = axis == 1 ? m->rows() : m->cols();
    double *sum = st.scratch.get<double>("mom_sum", std::max<uint64_t>(1, n));
    double *sumsq = st.scratch.get<double>("mom_sumsq", std::max<uint64_t>(1, n));
    axis_sums(m, axis, mode, sum, sumsq);
    s.resize(n);
    SCANRS_D2H(s.data(), sum, n * 8, st.stream);
    if (mode == 2) {
        s2.resize(n);
        SCANRS_D2H(s2.data(), sumsq, n * 8, st.stream);
    }
    SCANRS_SYNC(st.stream);
}

int scanrs_mat_center(scanrs_mat *m, int axis, const double *given_means) {
    return guard([&] { // sqz/src/mat.rs:937-962
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (axis != 0 && axis != 1) fail(SCANRS_ERR_ARGUMENT, "axis must be 0 or 1");
        if (m->off_rank) fail(SCANRS_ERR_ARGUMENT, "matrix already carries a low-rank offset");
        const uint64_t n = axis == 1 ? m->rows() : m->cols(), other = axis == 1 ? m->cols() : m->rows();
        std::vector<double> neg(n), s, s2;
        if (given_means) {
            for (uint64_t i = 0; i < n; i++) neg[i] = -given_means[i];
        } else {
            host_axis_sums(m, axis, 1, s, s2);
            const double ext = axis_extent(m, axis);
            for (uint64_t i = 0; i < n; i++) neg[i] = -(s[i] / ext);
        }
        std::vector<double> ones(other, 1.0);
        auto dn = upload_vec(*m->st, neg.data(), n), d1 = upload_vec(*m->st, ones.data(), other);
        if (axis == 1)
            set_offset_dev(m, 1, dn, d1);
        else
            set_offset_dev(m, 1, d1, dn);
    });
}
int scanrs_mat_scale(scanrs_mat *m, int axis, const double *given_std) {
    return guard([&] { // sqz/src/mat.rs:966-981
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (axis != 0 && axis != 1) fail(SCANRS_ERR_ARGUMENT, "axis must be 0 or 1");
        if (m->off_rank) fail(SCANRS_ERR_ARGUMENT, "cannot compose a map onto a LowRankOffset");
        const uint64_t n = axis == 1 ? m->rows() : m->cols();
        std::vector<double> f(n), s, s2;
        if (given_std) {
            for (uint64_t i = 0; i < n; i++) f[i] = 1.0 / given_std[i];
        } else {
            host_axis_sums(m, axis, 2, s, s2);
            const double ext = axis_extent(m, axis);
            for (uint64_t i = 0; i < n; i++) {
                const double mean = s[i] / ext;
                const double d = s2[i] / ext - mean * mean;
                f[i] = d == 0.0 ? 1.0 : 1.0 / std::sqrt(d);
            }
        }
        MapOp op;
        op.kind = OP_SCALE_AXIS;
        op.axis = 1 - axis;
        op.a = upload_vec(*m->st, f.data(), n);
        m->ops.push_back(op);
    });
}
int scanrs_mat_scale_and_center(scanrs_mat *m, int axis, const double *given_scaling) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        scale_and_center_impl(m, axis, given_scaling);
    });
}

int scanrs_mat_sum_axis_u32(scanrs_mat *m, int axis, uint32_t *out) {
    return guard([&] {
        if (!m || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (axis != 0 && axis != 1) fail(SCANRS_ERR_ARGUMENT, "axis must be 0 or 1");
        if (!map_is_raw(m)) fail(SCANRS_ERR_ARGUMENT, "u32 sums are defined on the raw count matrix");
        Storage &st = *m->st;
        if (st.shard.active() && (axis == 1 ? cols_sharded(m) : rows_sharded(m)))
            fail(SCANRS_ERR_ARGUMENT, "u32 sums over the sharded dimension are not supported");
        SparseCopy &cp = copy_outer_view_rows(m, axis == 1);
        DevMap raw;
        memset(&raw, 0, sizeof(raw));
        uint32_t *d = st.scratch.get<uint32_t>("sum_u32", std::max<uint64_t>(1, cp.n_outer));
        launch_row_reduce(st, cp, raw, 0, d, nullptr, nullptr);
        SCANRS_D2H(out, d, cp.n_outer * 4, st.stream);
        SCANRS_SYNC(st.stream);
    });
}
int scanrs_mat_sum_axis_f64(scanrs_mat *m, int axis, double *out) {
    return guard([&] {
        if (!m || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        std::vector<double> s, s2;
        host_axis_sums(m, axis, 1, s, s2);
        if (!s.empty()) memcpy(out, s.data(), s.size() * 8);
    });
}
int scanrs_mat_mean_axis(scanrs_mat *m, int axis, double *out) {
    return guard([&] {
        if (!m || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        std::vector<double> s, s2;
        host_axis_sums(m, axis, 1, s, s2);
        const double ext = axis_extent(m, axis);
        for (size_t i = 0; i < s.size(); i++) out[i] = s[i] / ext;
    });
}
int scanrs_mat_mean_var_axis(scanrs_mat *m, int axis, double *mean, double *var) {
    return guard([&] { // sqz/src/mat.rs:285-330
        if (!m || !mean || !var) fail(SCANRS_ERR_ARGUMENT, "null argument");
        std::vector<double> s, s2;
        host_axis_sums(m, axis, 2, s, s2);
        const double ext = axis_extent(m, axis);
        for (size_t i = 0; i < s.size(); i++) {
            mean[i] = s[i] / ext;
            var[i] = s2[i] / ext - mean[i] * mean[i];
        }
    });
}

int scanrs_mat_var_axis(scanrs_mat *m, int axis, double *var) {
    // sqz/src/mat.rs:409-411: mean_var_axis(axis).1 — through that very entry point, so the variances are the same bits
    if (!m || !var || (axis != 0 && axis != 1)) return guard([&] { fail(SCANRS_ERR_ARGUMENT, !m || !var ? "null argument" : "axis must be 0 or 1"); });
    std::vector<double> mean;
    const int rc = guard([&] { mean.resize(std::max<uint64_t>(1, axis == 1 ? m->rows() : m->cols())); });
    return rc != SCANRS_OK ? rc : scanrs_mat_mean_var_axis(m, axis, mean.data(), var);
}

int scanrs_mat_to_dense(scanrs_mat *m, double *out) {
    return guard([&] {
        if (!m || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        Storage &st = *m->st;
        const uint64_t R = m->rows(), C = m->cols();
        if (R * C == 0) return;
        double *d = st.scratch.get<double>("dense", R * C);
        SCANRS_HIP(hipMemsetAsync(d, 0, R * C * 8, st.stream));
        SparseCopy &cp = copy_outer_view_rows(m, true);
        launch_densify(st, cp, m->dev_map(true), true, C, d);
        SCANRS_D2H(out, d, R * C * 8, st.stream);
        if (m->off_rank) { // u.dot(&v) + mat  (low_rank_offset.rs:55-57)
            std::vector<double> u((size_t)R * m->off_rank), vt((size_t)C * m->off_rank);
            SCANRS_HIP(hipMemcpy(u.data(), m->off_u->p, u.size() * 8, hipMemcpyDeviceToHost));
            SCANRS_HIP(hipMemcpy(vt.data(), m->off_v->p, vt.size() * 8, hipMemcpyDeviceToHost));
            for (uint64_t r = 0; r < R; r++)
                for (uint64_t c = 0; c < C; c++) {
                    double acc = 0.0;
                    for (uint32_t q = 0; q < m->off_rank; q++) acc += u[r * m->off_rank + q] * vt[c * m->off_rank + q];
                    out[r * C + c] = acc + out[r * C + c];
                }
        }
    });
}

// ---- products -----------------------------------------------------------------------------------------------
static void dot_host(scanrs_mat *m, bool transpose, const double *h_in, uint32_t l, double *h_out, bool in_is_l_by_n) {
    // transpose = false: out[rows x l] = A * in[cols x l].   transpose = true (rdot): lhs is l x rows, out is l x cols:
    // computed as (A^T lhs^T)^T exactly like ArrayBase::dot(&AdaptiveMat) (sqz/src/mat.rs:1124-1132).
    CurrentHandle cur(m->st.get());
    dot_through_scratch(m, transpose, h_in, l, h_out, in_is_l_by_n, "dot_in", "dot_out",
                        [&](const double *dX, uint32_t ld, double *dY) { mat_apply(m, transpose, dX, ld, l, dY, ld); });
}

int scanrs_mat_dot(scanrs_mat *m, const double *rhs, uint32_t l, double *out) {
    return guard([&] {
        if (!m || (!rhs && l) || (!out && l)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        dot_host(m, false, rhs, l, out, false);
    });
}
int scanrs_mat_rdot(scanrs_mat *m, const double *lhs, uint32_t l, double *out) {
    return guard([&] {
        if (!m || (!lhs && l) || (!out && l)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        dot_host(m, true, lhs, l, out, true);
    });
}

static void dot_host_u32(scanrs_mat *m, bool transpose, const uint32_t *h_in, uint32_t l, uint32_t *h_out) {
    if (!map_is_raw(m) || m->off_rank) fail(SCANRS_ERR_ARGUMENT, "u32 products are defined on the raw count matrix");
    Storage &st = *m->st;
    CurrentHandle cur(&st);
    if (st.shard.active()) fail(SCANRS_ERR_ARGUMENT, "u32 products are not sharded");
    dot_through_scratch(m, transpose, h_in, l, h_out, transpose, "dotu_in", "dotu_out",
                        [&](const uint32_t *dX, uint32_t ld, uint32_t *dY) { launch_spmm_u32(st, copy_outer_view_rows(m, !transpose), dX, ld, l, dY, ld); });
}
int scanrs_mat_dot_u32(scanrs_mat *m, const uint32_t *rhs, uint32_t l, uint32_t *out) {
    return guard([&] {
        if (!m || (!rhs && l) || (!out && l)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        dot_host_u32(m, false, rhs, l, out);
    });
}
int scanrs_mat_rdot_u32(scanrs_mat *m, const uint32_t *lhs, uint32_t l, uint32_t *out) {
    return guard([&] {
        if (!m || (!lhs && l) || (!out && l)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        dot_host_u32(m, true, lhs, l, out);
    });
}
int scanrs_mat_dot_device(scanrs_mat *m, int transpose, const double *d_rhs, uint32_t ld_rhs, uint32_t l, double *d_out,
                          uint32_t ld_out) {
    return guard([&] {
        if (!m || !d_rhs || !d_out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        mat_apply(m, transpose != 0, d_rhs, ld_rhs, l, d_out, ld_out);
    });
}

// ---- normalization -------------------------------------------------------------------------------------------
int scanrs_log_normalize(scanrs_mat *m, double umi_count_sum, int log_fn, const uint32_t *size_factors) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        log_normalize_impl(m, umi_count_sum, log_fn, size_factors);
    });
}
int scanrs_log1p_normalize_fixed_point(scanrs_mat *m, int log_fn, uint32_t base, uint32_t exponent) {
    return guard([&] { // scan-rs/src/normalization.rs:191-213
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (!map_is_raw(m) || m->off_rank) fail(SCANRS_ERR_ARGUMENT, "needs the raw count matrix");
        if (log_fn != OP_LN_1P && log_fn != OP_LOG2_1P && log_fn != OP_LOG10_1P) fail(SCANRS_ERR_ARGUMENT, "bad log base");
        uint32_t p = 1; // fixed_point.base.pow(exponent) in u32
        for (uint32_t i = 0; i < exponent; i++) p *= base;
        std::vector<double> f(m->cols(), 1.0 / (double)p);
        MapOp sc;
        sc.kind = OP_SCALE_AXIS;
        sc.axis = 1;
        sc.a = upload_vec(*m->st, f.data(), f.size());
        m->ops.push_back(sc);
        MapOp lg;
        lg.kind = log_fn;
        m->ops.push_back(lg);
        scale_and_center_impl(m, 1, nullptr);
    });
}
// which product a solver runs second on this view: svd_bk / svd_rand start with A x when rows >= cols (bk_svd.rs:89, rand_svd.rs:86)
static void prefetch_for_pca(scanrs_mat *m) {
    const uint64_t Mg = rows_sharded(m) ? m->st->shard.outer_global : m->rows(), Ng = cols_sharded(m) ? m->st->shard.outer_global : m->cols();
    prepare_second_orientation(m, Mg >= Ng, true);
}

int scanrs_normalize(scanrs_mat *m, int normalization, const uint32_t *size_factors) {
    return guard([&] {
        stage_mark("normalize enter"); // normalize / normalize_with_size_factor, scan-rs/src/normalization.rs:46-102
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        const bool pca_next = normalization >= SCANRS_NORM_CELLRANGER && normalization <= SCANRS_NORM_LOG_TRANSFORM;
        if (pca_next && m->st->opt.side_build == 1) prefetch_for_pca(m); // 1: beside the normalisation passes; 2: right behind them
        switch (normalization) {
        case SCANRS_NORM_CELLRANGER:
            log_normalize_impl(m, -1.0, OP_LOG2_1P, nullptr);
            scale_and_center_impl(m, 1, nullptr);
            break;
        case SCANRS_NORM_CELLRANGER8: {
            log_normalize_impl(m, -1.0, OP_LOG2_1P, nullptr);
            std::vector<double> ones(m->rows(), 1.0);
            scale_and_center_impl(m, 1, ones.data());
            break;
        }
        case SCANRS_NORM_SEURATLOG:
            log_normalize_impl(m, 10000.0, OP_LN_1P, nullptr);
            scale_and_center_impl(m, 1, nullptr);
            break;
        case SCANRS_NORM_WITH_SIZE_FACTORS:
            log_normalize_impl(m, -1.0, OP_LOG2_1P, size_factors);
            scale_and_center_impl(m, 1, nullptr);
            break;
        case SCANRS_NORM_LOG_TRANSFORM: {
            std::vector<uint32_t> ones(m->cols(), 1u);
            log_normalize_impl(m, 1.0, OP_LOG2_1P, ones.data());
            scale_and_center_impl(m, 1, nullptr);
            break;
        }
        case SCANRS_NORM_BINOMIAL_DEVIANCE:
            binom_impl(m, OP_BINOM_DEV);
            break;
        case SCANRS_NORM_BINOMIAL_PEARSON:
            binom_impl(m, OP_BINOM_PEARSON);
            break;
        default:
            fail(SCANRS_ERR_ARGUMENT, "Normalization not recognized: %d", normalization);
        }
        if (pca_next && m->st->opt.side_build == 2) prefetch_for_pca(m);
    });
}
int scanrs_mat_target_umi(const scanrs_mat *m, double *target) {
    return guard([&] {
        if (!m || !target) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *target = m->target_umi;
    });
}

// ---- PCA ----------------------------------------------------------------------------------------------------------
int scanrs_pca_bk(scanrs_mat *m, uint32_t k, double k_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
                  const scanrs_snoop *snoop, double *u, double *s, double *v) {
    return guard([&] {
        if (!m || !s) fail(SCANRS_ERR_ARGUMENT, "null argument");
        stage_mark("pca_bk enter");
        pca_bk(m, k, k_multiplier, n_iter, seed, omega, snoop, u, s, v);
        device_free_flush(); // results delivered: the device is idle
        stage_mark("pca_bk leave");
    });
}
int scanrs_pca_rand(scanrs_mat *m, uint32_t k, double l_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
                    double *u, double *s, double *v) {
    return guard([&] {
        if (!m || !s) fail(SCANRS_ERR_ARGUMENT, "null argument");
        pca_rand(m, k, l_multiplier, n_iter, seed, omega, u, s, v);
        device_free_flush();
    });
}
int scanrs_pca_irlba(scanrs_mat *m, uint32_t nu, double tol, uint32_t max_iter, const double *v0, const scanrs_snoop *snoop,
                     double *u, double *s, double *v, uint32_t *mprod) {
    return guard([&] {
        if (!m || !u || !s || !v) fail(SCANRS_ERR_ARGUMENT, "null argument");
        pca_irlba(m, nu, tol, max_iter, v0, snoop, u, s, v, mprod);
        device_free_flush();
    });
}
int scanrs_pca_result_device(scanrs_mat *m, const double **d_u, uint32_t *ld_u, const double **d_v, uint32_t *ld_v, uint32_t *k) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        const Storage::PcaDev &r = m->st->pca_dev;
        if (!r.u || !r.v || r.k == 0) fail(SCANRS_ERR_ARGUMENT, "no PCA result on this handle yet");
        if (d_u) *d_u = r.u;
        if (ld_u) *ld_u = r.ld_u;
        if (d_v) *d_v = r.v;
        if (ld_v) *ld_v = r.ld_v;
        if (k) *k = r.k;
    });
}
int scanrs_omega_fill(uint64_t seed, uint64_t count, double *out) {
    return guard([&] {
        if (!out && count) fail(SCANRS_ERR_ARGUMENT, "null argument");
        omega_fill(seed, count, out);
    });
}

// ---- nearest neighbours (scan-rs/src/nn.rs) ------------------------------------------------------------------------------
int scanrs_knn(const double *points, uint64_t n, uint32_t d, uint32_t k, uint32_t *out) {
    return guard([&] {
        if ((!points && n) || (!out && n && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_device();
        knn_host(points, n, points, n, d, k, true, out);
    });
}
int scanrs_knn_device(const double *d_points, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, uint32_t *out) {
    return guard([&] {
        if ((!d_points && n) || (!out && n && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_device();
        knn_device(d_points, ld, n, d_points, ld, n, d, k, true, out);
    });
}
int scanrs_find_nn(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k, int include_self,
                   uint32_t *out) {
    return guard([&] {
        if ((!queries && n_q) || (!points && n_p) || (!out && n_q && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_device();
        knn_host(queries, n_q, points, n_p, d, k, include_self == 0, out);
    });
}
// rows [0, n_rows) of a host array (leading dimension ld >= d) into `buf`, through stream s and waited for: the array may be pageable
static const double *upload_rows(DevBuf<double> &buf, const double *rows, uint64_t n_rows, uint32_t ld, uint32_t d, hipStream_t s) {
    buf.alloc(std::max<uint64_t>(1, n_rows * ld));
    if (n_rows && ld >= d) {
        SCANRS_HIP(hipMemcpyAsync(buf.p, rows, ((n_rows - 1) * ld + d) * 8, hipMemcpyHostToDevice, s));
        SCANRS_SYNC(s);
    }
    return buf.p;
}
// The sharded half of scanrs_knn_sharded and scanrs_nearest_neighbors_sharded before their search: the refusals (`name` is the entry
// point's in their texts) and the rank's rows of the points in device memory. Host points span all the cells and only this rank's
// rows [begin, begin + n_local) go to the device (into `buf`); device points are the rank's own rows already.
static const double *rank_rows(scanrs_mat *m, const char *name, const double *points, int points_is_device, uint32_t ld, uint32_t d, bool no_out,
                               DevBuf<double> &buf) {
    const Storage &st = *m->st;
    const uint64_t n_local = m->cols();
    if (!cols_sharded(m)) fail(SCANRS_ERR_ARGUMENT, "%s: the cells (the columns of this view) must be the sharded dimension", name);
    if ((!points && (points_is_device ? n_local : st.shard.outer_global)) || (no_out && n_local)) fail(SCANRS_ERR_ARGUMENT, "null argument");
    return points_is_device ? points : upload_rows(buf, points + st.shard.outer_begin * ld, n_local, ld, d, st.stream);
}
// knn over a sharded handle: COLLECTIVE. The handle carries the transport and the rank's range of cells only.
int scanrs_knn_sharded(scanrs_mat *m, const double *points, int points_is_device, uint32_t ld, uint32_t d, uint32_t k, uint32_t *out,
                       double *sq_dist) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        CurrentHandle cur(m->st.get());
        Storage &st = *m->st;
        st.knn_blocks = st.knn_allreduces = 0;
        const uint64_t n_local = m->cols();
        DevBuf<double> buf;
        if (!st.shard.active()) { // scanrs_knn / scanrs_knn_device on the given points
            if ((!points && n_local) || (!out && n_local && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
            need_device();
            const bool upload = !points_is_device && n_local;
            if (upload && ld < d) fail(SCANRS_ERR_ARGUMENT, "knn: leading dimension smaller than the number of coordinates");
            const double *pts = upload ? upload_rows(buf, points, n_local, ld, d, 0) : points;
            knn_device(pts, ld, n_local, pts, ld, n_local, d, k, true, out, sq_dist);
            return;
        }
        const double *pts = rank_rows(m, "knn_sharded", points, points_is_device, ld, d, !out && k, buf);
        knn_sharded(st, pts, ld, st.shard.outer_begin, n_local, st.shard.outer_global, d, k, out, sq_dist);
        device_free_flush();
    });
}
int scanrs_host_knn_merge(uint32_t k, const double *da, const uint32_t *ia, const double *db, const uint32_t *ib, double *dout, uint32_t *iout) {
    return guard([&] {
        if (k && (!da || !ia || !db || !ib || !dout || !iout)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (k > 128) fail(SCANRS_ERR_ARGUMENT, "knn: k must not exceed 128");
        knn_host_merge(k, da, ia, db, ib, dout, iout);
    });
}
// ---- nearest_neighbors under Euclidean, Pearson and cosine distance (umap-rs/src/knn.rs:112-166, dist.rs) -----------------------
int scanrs_nearest_neighbors(const double *data, uint64_t n, uint32_t d, uint32_t k, int distance_type, uint32_t *indices, double *distances) {
    return guard([&] {
        if ((!data && n) || ((!indices || !distances) && n && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        nearest_neighbors_check_args(n, d, d, k, distance_type);
        if (k == 0 || n == 0) return;
        need_device();
        DevBuf<double> dp(n * d);
        SCANRS_HIP(hipMemcpy(dp.p, data, n * d * 8, hipMemcpyHostToDevice));
        nearest_neighbors_device(dp.p, n, d, d, k, distance_type, indices, distances);
    });
}
int scanrs_nearest_neighbors_device(const double *d_data, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int distance_type, uint32_t *indices,
                                    double *distances) {
    return guard([&] {
        if ((!d_data && n) || ((!indices || !distances) && n && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        nearest_neighbors_check_args(n, ld, d, k, distance_type);
        if (k == 0 || n == 0) return;
        need_device();
        nearest_neighbors_device(d_data, n, ld, d, k, distance_type, indices, distances);
    });
}
int scanrs_host_nearest_neighbors(const double *data, uint64_t n, uint32_t d, uint32_t k, int distance_type, uint32_t *indices, double *distances) {
    return guard([&] {
        if ((!data && n) || ((!indices || !distances) && n && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        host_nearest_neighbors(data, n, d, k, distance_type, indices, distances);
    });
}
// a query set of its own
int scanrs_nearest_neighbors_query(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k,
                                   int distance_type, int include_self, uint32_t *indices, double *distances) {
    return guard([&] {
        if ((!queries && n_q) || (!points && n_p) || ((!indices || !distances) && n_q && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        nearest_neighbors_check_args(n_p, d, d, k, distance_type);
        nearest_neighbors_check_args(n_q, d, d, k, distance_type);
        if (k == 0 || n_q == 0) return;
        need_device();
        const bool same = queries == points && n_q == n_p;
        DevBuf<double> dp(std::max<uint64_t>(1, n_p * d)), dq;
        if (n_p) SCANRS_HIP(hipMemcpy(dp.p, points, n_p * d * 8, hipMemcpyHostToDevice));
        if (!same) {
            dq.alloc(n_q * d);
            SCANRS_HIP(hipMemcpy(dq.p, queries, n_q * d * 8, hipMemcpyHostToDevice));
        }
        nearest_neighbors_query_device(same ? dp.p : dq.p, n_q, d, dp.p, n_p, d, d, k, distance_type, include_self != 0, indices, distances);
    });
}
int scanrs_nearest_neighbors_query_device(const double *d_queries, uint64_t n_q, uint32_t ld_q, const double *d_points, uint64_t n_p, uint32_t ld_p,
                                          uint32_t d, uint32_t k, int distance_type, int include_self, uint32_t *indices, double *distances) {
    return guard([&] {
        if ((!d_queries && n_q) || (!d_points && n_p) || ((!indices || !distances) && n_q && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        nearest_neighbors_check_args(n_p, ld_p, d, k, distance_type);
        nearest_neighbors_check_args(n_q, ld_q, d, k, distance_type);
        if (k == 0 || n_q == 0) return;
        need_device();
        nearest_neighbors_query_device(d_queries, n_q, ld_q, d_points, n_p, ld_p, d, k, distance_type, include_self != 0, indices, distances);
    });
}
int scanrs_host_nearest_neighbors_query(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k,
                                        int distance_type, int include_self, uint32_t *indices, double *distances) {
    return guard([&] {
        if ((!queries && n_q) || (!points && n_p) || ((!indices || !distances) && n_q && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        host_nearest_neighbors_query(queries, n_q, points, n_p, d, k, distance_type, include_self != 0, indices, distances);
    });
}
// nearest_neighbors over a sharded handle: COLLECTIVE, the argument conventions of scanrs_knn_sharded
int scanrs_nearest_neighbors_sharded(scanrs_mat *m, const double *points, int points_is_device, uint32_t ld, uint32_t d, uint32_t k,
                                     int distance_type, uint32_t *indices, double *distances) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        CurrentHandle cur(m->st.get());
        Storage &st = *m->st;
        st.knn_blocks = st.knn_allreduces = st.knn_blocks_filtered = 0;
        const uint64_t n_local = m->cols();
        DevBuf<double> buf;
        if (!st.shard.active()) { // scanrs_nearest_neighbors / _device on the given points
            if ((!points && n_local) || ((!indices || !distances) && n_local && k)) fail(SCANRS_ERR_ARGUMENT, "null argument");
            nearest_neighbors_check_args(n_local, ld, d, k, distance_type);
            if (k == 0 || n_local == 0) return;
            need_device();
            const double *pts = points_is_device ? points : upload_rows(buf, points, n_local, ld, d, 0);
            nearest_neighbors_device(pts, n_local, ld, d, k, distance_type, indices, distances);
            return;
        }
        const double *pts = rank_rows(m, "nearest_neighbors_sharded", points, points_is_device, ld, d, (!indices || !distances) && k, buf);
        nearest_neighbors_sharded(st, pts, ld, st.shard.outer_begin, n_local, st.shard.outer_global, d, k, distance_type, indices, distances);
        device_free_flush();
    });
}
int scanrs_host_distance(int distance_type, const double *x, const double *y, uint32_t d, double *key, double *dist) {
    return guard([&] {
        if (!x || !y || !key || !dist) fail(SCANRS_ERR_ARGUMENT, "null argument");
        nearest_neighbors_check_args(2, d, d, 1, distance_type);
        host_distance(distance_type, x, y, d, key, dist);
    });
}
int scanrs_host_metric_rows(int distance_type, const double *data, uint64_t n, uint32_t d, double *c, double *s, double *z) {
    return guard([&] {
        if (n && (!data || !c || !s)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        nearest_neighbors_check_args(n, d, d, 1, distance_type);
        if (distance_type == knn_metric::EUCLIDEAN) fail(SCANRS_ERR_ARGUMENT, "metric_rows: pearson (1) or cosine (2)");
        host_metric_rows(distance_type, data, n, d, c, s, z);
    });
}
int scanrs_debug_nearest_neighbors_params(double *delta, double *e, double *chain, double *sxx_min, double *sxx_max) {
    return guard([&] {
        if (!delta || !e || !chain || !sxx_min || !sxx_max) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *delta = knn_metric::KM_DELTA, *e = knn_metric::KM_E, *chain = knn_metric::KM_CHAIN;
        *sxx_min = knn_metric::KM_SXX_MIN, *sxx_max = knn_metric::KM_SXX_MAX;
    });
}
int scanrs_host_col_moments_plan(uint32_t max_count, uint32_t n_links, const int *kinds, const int *on_summed_axis, const double *fmin_pos,
                                 const double *fmax, uint64_t n_outer, uint64_t n_inner, uint32_t n_wg, int mode, int *accept, int *e1, int *e2) {
    return guard([&] {
        if (!accept || !e1 || !e2 || (n_links && (!kinds || !on_summed_axis || !fmin_pos || !fmax))) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (n_links > 64) fail(SCANRS_ERR_ARGUMENT, "col_moments_plan: at most 64 links");
        std::vector<col_moments::Link> links(n_links);
        for (uint32_t i = 0; i < n_links; i++) links[i] = {kinds[i], on_summed_axis[i], fmin_pos[i], fmax[i]};
        const col_moments::Plan p = col_moments::plan(max_count, links.data(), (int)n_links, n_outer, n_inner, n_wg, mode);
        *accept = p.ok ? 1 : 0;
        *e1 = p.e1;
        *e2 = p.e2;
    });
}
int scanrs_host_spmm_route(const double *options, uint64_t n_outer, uint64_t n_inner, uint64_t nnz, uint32_t l, uint32_t ldx, uint32_t n_links,
                           const int *kinds, const int *a_outer, uint32_t flags, uint64_t *out) {
    return guard([&] {
        if (!options || !out || (n_links && (!kinds || !a_outer))) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (n_links > (uint32_t)MAX_OPS) fail(SCANRS_ERR_ARGUMENT, "spmm_route: at most %d links", MAX_OPS);
        SpmmQuery q;
        options_from_route_array(options, q.o);
        q.n_outer = n_outer, q.n_inner = n_inner, q.nnz = nnz, q.l = l, q.ldx = ldx;
        q.n_links = (int)n_links;
        for (uint32_t j = 0; j < n_links; j++) q.kind[j] = kinds[j], q.a_outer[j] = a_outer[j] != 0;
        q.values_room = (flags & SCANRS_SPMM_NO_VALUES_ROOM) == 0;
        const SpmmRoute r = spmm_route(q, (flags & SCANRS_SPMM_TILES_AVAILABLE) != 0);
        out[0] = (uint64_t)r.family, out[1] = r.form_bits(), out[2] = r.chunk_bits(), out[3] = r.family == SPMM_TILES ? r.chunk_width : 0, out[4] = r.even_ld ? 1 : 0;
        out[5] = tiles_static_candidate(q) ? 1 : 0;
    });
}
int scanrs_host_bk_plan(const double *colmax, uint64_t n, uint32_t b, uint32_t n_iter, double reuse_cmax, int coef_valid, uint64_t *out,
                        double *limit, double *cmax_dense, uint32_t *direct) {
    return guard([&] {
        if (!colmax || !out || !limit || !cmax_dense || !direct) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (b == 0 || n_iter == 0) fail(SCANRS_ERR_ARGUMENT, "bk_plan: b and n_iter must be positive");
        if (n != (uint64_t)b * n_iter || n > 0xFFFFFFFFull) fail(SCANRS_ERR_ARGUMENT, "bk_plan: colmax must hold b * n_iter entries");
        for (uint64_t j = 0; j < n; j++)
            if (!std::isfinite(colmax[j]) || colmax[j] < 0.0) fail(SCANRS_ERR_ARGUMENT, "bk_plan: colmax must be finite and non-negative");
        if (!(reuse_cmax > 0.0)) fail(SCANRS_ERR_ARGUMENT, "reuse_cmax must be positive");
        const BkPlan p = bk_plan(colmax, b, n_iter, reuse_cmax, coef_valid != 0);
        out[0] = p.reuse, out[1] = p.flagged_older, out[2] = (uint64_t)p.limit_branch, out[3] = p.direct.size(), out[4] = p.last_direct;
        out[5] = p.full_direct, out[6] = p.n_early;
        *limit = p.limit, *cmax_dense = p.cmax_dense;
        std::copy(p.direct.begin(), p.direct.end(), direct);
    });
}
int scanrs_host_transpose_plan(uint64_t n_outer, uint64_t n_inner, uint32_t max_value, int *route, uint32_t *ib, uint32_t *ob, uint32_t *cb) {
    return guard([&] {
        if (!route || !ib || !ob || !cb) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (n_outer > 0xFFFFFFFFull || n_inner > 0xFFFFFFFFull) fail(SCANRS_ERR_SHAPE, "dimensions must fit in u32 (AdaptiveVec limit)");
        const TransposePlan p = transpose_plan(n_outer, n_inner, max_value);
        *route = (int)p.route, *ib = p.ib, *ob = p.ob, *cb = p.cb;
    });
}
int scanrs_debug_knn_filter(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, const double *tau,
                            uint64_t stride, uint32_t *cnt, uint32_t *cand) {
    return guard([&] {
        if (!queries || !points || !tau || !cnt || !cand) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_device();
        knn_filter_debug(queries, n_q, points, n_p, d, tau, stride, cnt, cand);
    });
}
int scanrs_debug_knn_last_stats(int *filtered, uint64_t *first_stride, uint32_t *n_rounds, uint32_t capacity, uint64_t *strides, uint64_t *points,
                                uint64_t *cand_sum, uint32_t *cand_max, uint32_t *overflowed) {
    return guard([&] {
        if (!filtered || !first_stride || !n_rounds) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (capacity && (!strides || !points || !cand_sum || !cand_max || !overflowed)) fail(SCANRS_ERR_ARGUMENT, "null array");
        bool f = false;
        std::vector<uint64_t> st, np, cs;
        std::vector<uint32_t> cm, ov;
        knn_last_stats(f, *first_stride, st, np, cs, cm, ov);
        *filtered = f ? 1 : 0;
        *n_rounds = (uint32_t)st.size();
        for (uint32_t i = 0; i < capacity && i < st.size(); i++) {
            strides[i] = st[i];
            points[i] = np[i];
            cand_sum[i] = cs[i];
            cand_max[i] = cm[i];
            overflowed[i] = ov[i];
        }
    });
}
int scanrs_debug_knn_filter_params(double *gamma, uint32_t *cap, uint32_t *dmax, uint32_t *k_max, uint64_t *nq_min, double *coord_min,
                                   double *coord_max) {
    return guard([&] {
        if (!gamma || !cap || !dmax || !k_max || !nq_min || !coord_min || !coord_max) fail(SCANRS_ERR_ARGUMENT, "null argument");
        knn_filter_params(*gamma, *cap, *dmax, *k_max, *nq_min, *coord_min, *coord_max);
    });
}

// ---- multi-GPU ----------------------------------------------------------------------------------------------------
int scanrs_mat_set_shard(scanrs_mat *m, uint32_t rank, uint32_t world, uint64_t outer_begin, uint64_t outer_global,
                         scanrs_allreduce_fn allreduce, void *ctx) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (world == 0 || rank >= world) fail(SCANRS_ERR_ARGUMENT, "bad rank/world");
        if (world > 1 && !allreduce) fail(SCANRS_ERR_ARGUMENT, "an all-reduce callback is required when world > 1");
        Storage &st = *m->st;
        if (outer_begin + st.primary.n_outer > outer_global) fail(SCANRS_ERR_SHAPE, "shard exceeds the global extent");
        st.shard.rank = rank;
        st.shard.world = world;
        st.shard.outer_begin = outer_begin;
        st.shard.outer_global = outer_global;
        st.shard.allreduce = allreduce;
        st.shard.ctx = ctx;
        st.shard.comm = nullptr;
    });
}
int scanrs_mat_set_shard_comm(scanrs_mat *m, scanrs_comm *comm, uint32_t rank, uint32_t world, uint64_t outer_begin,
                              uint64_t outer_global) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (world == 0 || rank >= world) fail(SCANRS_ERR_ARGUMENT, "bad rank/world");
        if (world > 1 && !comm) fail(SCANRS_ERR_ARGUMENT, "a communicator is required when world > 1");
        Storage &st = *m->st;
        if (outer_begin + st.primary.n_outer > outer_global) fail(SCANRS_ERR_SHAPE, "shard exceeds the global extent");
        st.shard.rank = rank;
        st.shard.world = world;
        st.shard.outer_begin = outer_begin;
        st.shard.outer_global = outer_global;
        st.shard.allreduce = nullptr;
        st.shard.ctx = nullptr;
        st.shard.comm = comm;
    });
}
int scanrs_plan_shards(const uint64_t *indptr, uint64_t n_outer, uint32_t world, uint64_t *bounds) {
    return guard([&] {
        if (!indptr || !bounds || world == 0) fail(SCANRS_ERR_ARGUMENT, "bad argument");
        const uint64_t nnz = indptr[n_outer] - indptr[0];
        bounds[0] = 0;
        for (uint32_t r = 1; r < world; r++) {
            // first outer index whose prefix reaches r/world of the nonzeros
            const uint64_t want = indptr[0] + (uint64_t)(((long double)nnz * r) / world);
            const uint64_t *p = std::lower_bound(indptr, indptr + n_outer + 1, want);
            uint64_t b = (uint64_t)(p - indptr);
            b = std::min(b, n_outer);
            bounds[r] = std::max(b, bounds[r - 1]);
        }
        bounds[world] = n_outer;
    });
}

// ---- measurement ------------------------------------------------------------------------------------------------------
int scanrs_profile_enable(scanrs_mat *m, int on) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        m->st->prof.on = on != 0;
    });
}
int scanrs_profile_reset(scanrs_mat *m) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        SCANRS_SYNC(m->st->stream);
        m->st->prof.reset();
    });
}
int scanrs_profile_get(scanrs_mat *m, scanrs_kernel_stat *out, uint32_t cap, uint32_t *n) {
    return guard([&] {
        if (!m || !n) fail(SCANRS_ERR_ARGUMENT, "null argument");
        SCANRS_SYNC(m->st->stream);
        m->st->prof.resolve();
        uint32_t i = 0;
        for (auto &kv : m->st->prof.stats) {
            if (out && i < cap) {
                memset(&out[i], 0, sizeof(out[i]));
                strncpy(out[i].name, kv.first.c_str(), sizeof(out[i].name) - 1);
                out[i].launches = kv.second.launches;
                out[i].total_ms = kv.second.ms;
                out[i].algorithmic_bytes = kv.second.bytes;
                out[i].onchip_gather_bytes = kv.second.onchip;
            }
            i++;
        }
        *n = i;
    });
}
int scanrs_mat_create_from_file(const char *path, const char *retain_feature_like, int64_t shrink_row, scanrs_mat **out,
                                scanrs_h5_matrix **meta) {
    if (out) *out = nullptr;
    if (meta) *meta = nullptr;
    if (!path || !out) return guard([&] { fail(SCANRS_ERR_ARGUMENT, "null argument"); });
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
    rc = scanrs_mat_create(rows, cols, storage, ip, ix, vv, out);
    if (rc == SCANRS_OK && meta)
        *meta = h;
    else
        scanrs_h5_matrix_free(h);
    return rc;
}
int scanrs_mat_sync(scanrs_mat *m) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        CurrentHandle cur(m->st.get(), true);
        SCANRS_SYNC(m->st->stream);
        device_free_flush();
    });
}

// One pass of the device-side CholeskyQR factor step on a host matrix (tests / diagnostics; the solvers queue the same
// kernel between a Gram kernel and a GEMM without looking at its verdict until the Krylov basis is complete).
int scanrs_mat_chol_rinv(scanrs_mat *m, const double *g, uint32_t n, uint64_t rows, int pass, double *rinv, int *done, int *status,
                         double *err, double *shift) {
    return guard([&] {
        if (!m || !g || !rinv) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (!chol_rinv_ok(n)) fail(SCANRS_ERR_ARGUMENT, "n must be in 1..128");
        if (rows == 0 || rows > (1ull << 40)) fail(SCANRS_ERR_ARGUMENT, "rows must be in 1..2^40 (it scales the shift of the factor step)");
        Storage &st = *m->st;
        double *dG = st.scratch.get<double>("chk_G", (size_t)n * n), *dR = st.scratch.get<double>("chk_R", (size_t)n * n);
        double *dInfo = st.scratch.get<double>("chk_info", 2);
        int *dCtl = st.scratch.get<int>("chk_ctl", 2);
        SCANRS_HIP(hipMemcpyAsync(dG, g, (size_t)n * n * 8, hipMemcpyHostToDevice, st.stream));
        SCANRS_HIP(hipMemsetAsync(dCtl, 0, 2 * sizeof(int), st.stream));
        SCANRS_HIP(hipMemsetAsync(dInfo, 0, 2 * sizeof(double), st.stream));
        launch_chol_rinv(st, dG, n, rows, pass, false, dCtl, dR, dInfo);
        int ctl[2];
        double info[2];
        SCANRS_D2H(rinv, dR, (size_t)n * n * 8, st.stream);
        SCANRS_D2H(ctl, dCtl, sizeof ctl, st.stream);
        SCANRS_D2H(info, dInfo, sizeof info, st.stream);
        if (done) *done = ctl[0];
        if (status) *status = ctl[1];
        if (err) *err = info[0];
        if (shift) *shift = info[1];
    });
}

// ---- the dense products one kernel at a time (tests): host arrays in, the WHOLE output buffer back, padding included -----------
} // extern "C"
namespace {
constexpr uint64_t DBG_MAX_ELEMS = 1ull << 26; // doubles per uploaded array (512 MB)
uint64_t dbg_count(uint64_t rows, uint32_t ld) {
    if (rows == 0 || ld == 0 || rows > DBG_MAX_ELEMS / ld) fail(SCANRS_ERR_ARGUMENT, "array of %llu x %u doubles: empty or too large", (unsigned long long)rows, ld);
    return rows * ld;
}
double *dbg_upload(Storage &st, const char *key, const double *h, uint64_t count, uint64_t skew = 0) {
    double *d = st.scratch.get<double>(key, count + 2) + skew;
    SCANRS_HIP(hipMemcpyAsync(d, h, count * 8, hipMemcpyHostToDevice, st.stream));
    return d;
}
// Storage::skip_flag pointing at a device int that holds 1 for the lifetime of the object; restored also when an error unwinds
struct DbgSkip {
    Storage &st;
    const int *saved;
    DbgSkip(Storage &s, bool on) : st(s), saved(s.skip_flag) {
        if (!on) return;
        int *flag = st.scratch.get<int>("dbg_skip", 1);
        const int one = 1;
        SCANRS_HIP(hipMemcpyAsync(flag, &one, sizeof one, hipMemcpyHostToDevice, st.stream));
        st.skip_flag = flag;
    }
    ~DbgSkip() { st.skip_flag = saved; }
};
} // namespace
extern "C" {
int scanrs_debug_dense_route(int kind, uint32_t n, uint32_t m, uint64_t rows, uint32_t ldx, uint32_t ldy, int x_aligned16, int side, int flag,
                             int *route, uint32_t *nt, uint32_t *groups) {
    return guard([&] {
        if (!route || !nt || !groups) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (kind == 0) {
            *route = gram_route(n, m, rows, ldx, ldy, side != 0, flag != 0);
            *nt = *groups = 0;
        } else if (kind == 1) {
            if (ldx & 1u) fail(SCANRS_ERR_ARGUMENT, "gemm: ldx must be even");
            const GemmPlan p = gemm_route(x_aligned16 != 0, ldx, n, m, rows, side != 0, flag != 0);
            *route = p.route;
            *nt = p.nt;
            *groups = p.groups;
        } else {
            fail(SCANRS_ERR_ARGUMENT, "kind must be 0 (Gram) or 1 (GEMM)");
        }
    });
}
int scanrs_debug_dense_gram(scanrs_mat *m, int route, const double *x, uint32_t ldx, uint32_t n, const double *y, uint32_t ldy, uint32_t mcols,
                            uint64_t rows, uint64_t rows_alloc, int skip, double *c) {
    return guard([&] {
        if (!m || !x || !c) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (n == 0 || mcols == 0 || rows == 0 || rows_alloc < rows || ldx < n || ldy < mcols) fail(SCANRS_ERR_ARGUMENT, "bad shape");
        if (!y && (mcols != n || ldy != ldx)) fail(SCANRS_ERR_ARGUMENT, "y == NULL (Y is X) needs mcols == n and ldy == ldx");
        need_device();
        Storage &st = *m->st;
        CurrentHandle cur(&st);
        const uint64_t nx = dbg_count(rows_alloc, ldx), ny = dbg_count(rows_alloc, ldy), nc = dbg_count(n, mcols);
        const double *dX = dbg_upload(st, "dbg_X", x, nx);
        const double *dY = y ? dbg_upload(st, "dbg_Y", y, ny) : dX;
        double *dC = dbg_upload(st, "dbg_C", c, nc);
        {
            DbgSkip sk(st, skip != 0);
            launch_gram_route(st, route, dX, ldx, n, dY, ldy, mcols, rows, dC);
        }
        SCANRS_D2H(c, dC, nc * 8, st.stream);
    });
}
int scanrs_debug_dense_gemm(scanrs_mat *m, int route, const double *x, int x_skew, uint32_t ldx, uint32_t n, const double *w, uint32_t ldw,
                            uint32_t mcols, uint64_t rows, uint64_t rows_alloc, double alpha, double beta, const double *cin, uint32_t ldc, double *out,
                            uint32_t ldo, int in_place, int skip) {
    return guard([&] {
        if (!m || !x || !w || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (n == 0 || mcols == 0 || rows == 0 || rows_alloc < rows || ldx < n || ldw < mcols || ldo < mcols) fail(SCANRS_ERR_ARGUMENT, "bad shape");
        if (x_skew != 0 && x_skew != 1) fail(SCANRS_ERR_ARGUMENT, "x_skew must be 0 or 1");
        if (in_place ? ldc != ldo : (cin ? ldc < mcols : beta != 0.0)) fail(SCANRS_ERR_ARGUMENT, "cin: in place needs ldc == ldo, a separate one ldc >= mcols, none beta == 0");
        const uint64_t nx = dbg_count(rows_alloc, ldx), nw = dbg_count(n, ldw), no = dbg_count(rows_alloc, ldo);
        const uint64_t ncin = (!in_place && cin) ? dbg_count(rows_alloc, ldc) : 0;
        if (x < out + no && out < x + nx) fail(SCANRS_ERR_ARGUMENT, "out overlaps x");
        need_device();
        Storage &st = *m->st;
        CurrentHandle cur(&st);
        const double *dX = dbg_upload(st, "dbg_X", x, nx, (uint64_t)x_skew);
        const double *dW = dbg_upload(st, "dbg_W", w, nw);
        double *dOut = dbg_upload(st, "dbg_Out", out, no);
        const double *dCin = in_place ? dOut : (cin ? dbg_upload(st, "dbg_Cin", cin, ncin) : nullptr);
        {
            DbgSkip sk(st, skip != 0);
            launch_gemm_route(st, route, dX, ldx, n, dW, ldw, mcols, rows, alpha, beta, dCin, ldc, dOut, ldo);
        }
        SCANRS_D2H(out, dOut, no * 8, st.stream);
    });
}
int scanrs_debug_weighted_colsum(scanrs_mat *m, const double *b, uint32_t rank, const double *x, uint32_t ldx, uint64_t n, uint32_t l, double *w,
                                 uint32_t ldw, double *xc, uint32_t ldc) {
    return guard([&] {
        if (!m || !b || !x || !w) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (rank == 0 || l == 0 || n == 0 || ldw < l || (ldx & 1u) || ldx < even_up(l)) fail(SCANRS_ERR_ARGUMENT, "bad shape (ldx even and >= l rounded up to even)");
        if (xc && ((l & 1u) || (ldc & 1u) || ldc < l)) fail(SCANRS_ERR_ARGUMENT, "xc needs l and ldc even, ldc >= l");
        need_device();
        Storage &st = *m->st;
        CurrentHandle cur(&st);
        const uint64_t nb = dbg_count(n, rank), nx = dbg_count(n, ldx), nw = dbg_count(rank, ldw), nxc = xc ? dbg_count(n, ldc) : 0;
        const double *dB = dbg_upload(st, "dbg_B", b, nb);
        const double *dX = dbg_upload(st, "dbg_X", x, nx);
        double *dW = dbg_upload(st, "dbg_W", w, nw);
        double *dXc = xc ? dbg_upload(st, "dbg_Xc", xc, nxc) : nullptr;
        launch_weighted_colsum(st, dB, rank, dX, ldx, n, l, dW, ldw, dXc, ldc);
        SCANRS_D2H(w, dW, nw * 8, st.stream);
        if (xc) SCANRS_D2H(xc, dXc, nxc * 8, st.stream);
    });
}

// ---- host-only utilities exposed for the CPU test-suite (no device needed) --------------------------------------------
int scanrs_debug_arena_selftest(uint32_t rounds, uint64_t seed) {
    return guard([&] { reserve_selftest(rounds, seed); });
}
int scanrs_host_chol_upper(double *g, int n) { return chol_upper(g, n) ? 0 : SCANRS_ERR_NUMERICAL; }
int scanrs_host_inv_upper(double *r, int n) {
    inv_upper(r, n);
    return 0;
}
int scanrs_host_sym_eig(const double *a, int n, double *w, double *z) { return sym_eig(a, n, w, z) ? 0 : SCANRS_ERR_NUMERICAL; }
int scanrs_host_sym_eig_topk(const double *a, int n, int k, double *w, double *z) {
    return sym_eig_topk(a, n, k, w, z) ? 0 : SCANRS_ERR_NUMERICAL;
}

} // extern "C"

// ---- select_rows / select_cols / partition_on_thresholds / to_csmat (select_host.cpp / select.hip) --------------------------------------
extern "C" {
int scanrs_mat_select_rows(scanrs_mat *m, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out) {
    return guard([&] { select_axis(m, true, idx, n_idx, out); });
}
int scanrs_mat_select_cols(scanrs_mat *m, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out) {
    return guard([&] { select_axis(m, false, idx, n_idx, out); });
}
// the plain entry point and the collective one of a sharded handle: the lists along the sharded dimension span the whole matrix
static void partition_entry(scanrs_mat *m, const double *row_threshold, const double *col_threshold, scanrs_mat **filtered, scanrs_mat **residual,
                            uint64_t *selected_rows, uint64_t *n_selected_rows, uint64_t *selected_cols, uint64_t *n_selected_cols, bool collective) {
    if (filtered) *filtered = nullptr;
    if (residual) *residual = nullptr;
    if (!m || !selected_rows || !n_selected_rows || !selected_cols || !n_selected_cols) fail(SCANRS_ERR_ARGUMENT, "null argument");
    need_device();
    need_plain_unsharded(m, "partition_on_thresholds", collective);
    Storage &st = *m->st;
    const bool outer_is_view_rows = (st.storage == SCANRS_CSR) != m->transposed;
    const int view_storage = m->transposed ? 1 - st.storage : st.storage;
    const bool sharded = st.shard.active();
    SparseCopy f, r;
    std::vector<uint8_t> ex_outer, ex_inner;
    PartitionShard ps;
    {
        CurrentHandle cur(&st);
        st.partition_allreduces = 0;
        st.partition_rounds = partition_on_thresholds(st, st.primary, outer_is_view_rows ? row_threshold : col_threshold,
                                                      outer_is_view_rows ? col_threshold : row_threshold, outer_is_view_rows, ex_outer, ex_inner,
                                                      filtered ? &f : nullptr, residual ? &r : nullptr, sharded ? &ps : nullptr);
        device_free_flush();
    }
    const std::vector<uint8_t> &ex_outer_all = sharded ? ps.excl_outer_all : ex_outer;
    const std::vector<uint8_t> &ex_rows = outer_is_view_rows ? ex_outer_all : ex_inner, &ex_cols = outer_is_view_rows ? ex_inner : ex_outer_all;
    uint64_t nr = 0, nc = 0;
    for (uint64_t i = 0; i < ex_rows.size(); i++)
        if (!ex_rows[i]) selected_rows[nr++] = i;
    for (uint64_t i = 0; i < ex_cols.size(); i++)
        if (!ex_cols[i]) selected_cols[nc++] = i;
    *n_selected_rows = nr;
    *n_selected_cols = nc;
    scanrs_mat *hf = filtered ? adopt_copy(made_rows(f, view_storage), made_cols(f, view_storage), view_storage, std::move(f)) : nullptr;
    scanrs_mat *hr = nullptr;
    try {
        if (residual) hr = adopt_copy(made_rows(r, view_storage), made_cols(r, view_storage), view_storage, std::move(r));
    } catch (...) {
        scanrs_mat_free(hf);
        throw;
    }
    if (sharded) {
        // where this rank's results lie: the kept (excluded) outer vectors below its own first one, and their number in the whole matrix.
        // The residual holds the kept rows x the excluded columns: the excluded outer vectors when the columns are the outer dimension.
        uint64_t kept_below = 0, kept_all = 0;
        for (uint64_t o = 0; o < ex_outer_all.size(); o++) {
            if (ex_outer_all[o]) continue;
            kept_all++;
            if (o < st.shard.outer_begin) kept_below++;
        }
        const uint64_t gone_below = st.shard.outer_begin - kept_below, gone_all = ex_outer_all.size() - kept_all;
        if (hf) bind_like(st, hf, kept_below, kept_all);
        if (hr) bind_like(st, hr, outer_is_view_rows ? kept_below : gone_below, outer_is_view_rows ? kept_all : gone_all);
    }
    if (residual) *residual = hr;
    if (filtered) *filtered = hf;
}
int scanrs_mat_partition_on_thresholds(scanrs_mat *m, const double *row_threshold, const double *col_threshold, scanrs_mat **filtered,
                                       scanrs_mat **residual, uint64_t *selected_rows, uint64_t *n_selected_rows, uint64_t *selected_cols,
                                       uint64_t *n_selected_cols) {
    return guard([&] {
        partition_entry(m, row_threshold, col_threshold, filtered, residual, selected_rows, n_selected_rows, selected_cols, n_selected_cols, false);
    });
}
// The collective forms: every rank of a sharded handle calls them with the same arguments; on an unsharded handle they are
// the plain calls.
int scanrs_mat_select_rows_sharded(scanrs_mat *m, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out) {
    return guard([&] { select_axis(m, true, idx, n_idx, out, true); });
}
int scanrs_mat_select_cols_sharded(scanrs_mat *m, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out) {
    return guard([&] { select_axis(m, false, idx, n_idx, out, true); });
}
int scanrs_mat_partition_on_thresholds_sharded(scanrs_mat *m, const double *row_threshold, const double *col_threshold, scanrs_mat **filtered,
                                               scanrs_mat **residual, uint64_t *selected_rows, uint64_t *n_selected_rows,
                                               uint64_t *selected_cols, uint64_t *n_selected_cols) {
    return guard([&] {
        partition_entry(m, row_threshold, col_threshold, filtered, residual, selected_rows, n_selected_rows, selected_cols, n_selected_cols, true);
    });
}
int scanrs_mat_shard_info(const scanrs_mat *m, uint32_t *rank, uint32_t *world, uint64_t *outer_begin, uint64_t *outer_global) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null argument");
        const Storage &st = *m->st;
        const bool sharded = st.shard.active();
        if (rank) *rank = sharded ? st.shard.rank : 0u;
        if (world) *world = sharded ? st.shard.world : 1u;
        if (outer_begin) *outer_begin = sharded ? st.shard.outer_begin : 0ull;
        if (outer_global) *outer_global = sharded ? st.shard.outer_global : st.primary.n_outer;
    });
}
int scanrs_mat_to_csmat(scanrs_mat *m, uint64_t *indptr, uint32_t *indices, uint32_t *values) {
    return guard([&] {
        if (!m || !indptr) fail(SCANRS_ERR_ARGUMENT, "null argument");
        Storage &st = *m->st;
        const SparseCopy &cp = st.primary; // a transposed view's storage flag is the other one: the same arrays
        if (cp.nnz && (!indices || !values)) fail(SCANRS_ERR_ARGUMENT, "null indices/values");
        CurrentHandle cur(&st);
        SCANRS_D2H(indptr, cp.indptr.p, (cp.n_outer + 1) * 8, st.stream);
        if (cp.nnz) {
            SCANRS_D2H(indices, cp.indices.p, cp.nnz * 4, st.stream);
            SCANRS_D2H(values, cp.values.p, cp.nnz * 4, st.stream);
        }
        SCANRS_SYNC(st.stream);
    });
}
} // extern "C"
