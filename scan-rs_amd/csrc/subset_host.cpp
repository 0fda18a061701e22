// Host side of sum_rows / sum_cols / sum_rows_dual / mean_rows / mean_var_rows (sqz/src/mat.rs:279-282, 333-374, 414-583): the
// checks of the lists, the choice of the copy and of the kernel form, and the entry points. Kernels: subset.hip.
//
// Which form runs (rows and columns are the view's; "row copy" = the copy whose outer vectors are the view's rows):
//
//   result per row    (sum_rows*, mean_rows, mean_var_rows)   row copy exists      masked walk over the row copy
//                                                             only the column copy u64: listed vectors of the column copy, scattered
//                                                                                  f64, or "subset_scatter" 0: the row copy is built
//   result per listed column (sum_cols*)                      column copy exists   listed vectors of the column copy
//                                                             only the row copy    u64: masked walk of the row copy, scattered
//                                                                                  f64, or "subset_scatter" 0: the column copy is built
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace scanrs {

namespace {

void subset_progress(const scanrs_snoop *sn, double p) {
    // CancelProgress::set_progress_check (snoop/src/lib.rs:45-57)
    if (!sn) return;
    if (sn->cancel && __atomic_load_n(sn->cancel, __ATOMIC_RELAXED)) fail(SCANRS_ERR_CANCELLED, "cancellation error");
    if (sn->progress) sn->progress(sn->ctx, p);
}

bool map_is_raw(const scanrs_mat *m) {
    for (const auto &op : m->ops)
        if (op.kind != OP_INTO) return false;
    return true;
}

// "must be sorted" (mat.rs:413, 448); as scanrs_sseq_params' cell list, a repeated index is refused too
void check_list(const uint64_t *l, uint64_t n, uint64_t extent, const char *name) {
    if (n && !l) fail(SCANRS_ERR_ARGUMENT, "%s: null index list", name);
    for (uint64_t i = 0; i < n; i++) {
        if (l[i] >= extent)
            fail(SCANRS_ERR_ARGUMENT, "%s: entry %llu is %llu, the matrix has %llu columns", name, (unsigned long long)i, (unsigned long long)l[i],
                 (unsigned long long)extent);
        if (i && l[i] <= l[i - 1])
            fail(SCANRS_ERR_ARGUMENT, "%s must be strictly ascending: entry %llu is %llu after %llu", name, (unsigned long long)i,
                 (unsigned long long)l[i], (unsigned long long)l[i - 1]);
    }
}

struct List {
    const uint64_t *idx;
    uint64_t n;
    const char *name;
};

// per_column false: out[k] (rows entries) = sums of every row over list k. per_column true (one list): out[0] (n entries) = the sums
// of the listed columns over all rows. mode 0: u64 of the raw counts; 1: f64 of the mapped values; 2: out[0] = sums, out[1] = sums of
// squares of the mapped values over the one list.
void subset_sums(scanrs_mat *m, bool per_column, int mode, const List *lists, int n_lists, const scanrs_snoop *snoop, void *const *out) {
    if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
    Storage &st = *m->st;
    const uint64_t rows = m->rows(), cols = m->cols();
    const uint64_t n_result = per_column ? lists[0].n : rows;
    const int n_out = mode == 2 ? 2 : n_lists;
    for (int k = 0; k < n_out; k++)
        if (n_result && !out[k]) fail(SCANRS_ERR_ARGUMENT, "null argument");
    if (st.shard.active()) fail(SCANRS_ERR_ARGUMENT, "sums over a column list of a sharded handle are not supported");
    if (mode == 0 && !map_is_raw(m)) fail(SCANRS_ERR_ARGUMENT, "u64 sums are defined on the raw count matrix");
    uint64_t n_all = 0;
    for (int k = 0; k < n_lists; k++) {
        check_list(lists[k].idx, lists[k].n, cols, lists[k].name);
        n_all += lists[k].n;
    }
    subset_progress(snoop, 0.0); // (a flag that is already set: nothing has been queued, the outputs are untouched)

    CurrentHandle cur(&st);
    hipStream_t s = st.stream;
    // the copy whose outer dimension is the result axis: does it exist? (other_settled, not has_other: the route must not depend on
    // how far a helper thread has come)
    const bool want_base_rows = (!per_column) != m->transposed;
    const bool exists = want_base_rows == (st.storage == SCANRS_CSR) || st.other_settled;
    const bool scatter = !exists && mode == 0 && st.subset_scatter != 0;
    SparseCopy &cp = scatter ? st.primary : st.copy_with_outer_rows(want_base_rows);
    const bool outer_is_view_row = scatter ? per_column : !per_column;
    const bool listed_outer = !outer_is_view_row; // the lists name view columns

    // the lists, narrowed to u32, through the pinned staging buffer
    uint32_t *d_lists = st.scratch.get<uint32_t>("subset_lists", std::max<uint64_t>(1, n_all));
    const uint32_t *d_list[2] = {d_lists, d_lists + lists[0].n};
    if (n_all) {
        uint32_t *h = static_cast<uint32_t *>(st.pinned(n_all * 4));
        uint64_t at = 0;
        for (int k = 0; k < n_lists; k++)
            for (uint64_t i = 0; i < lists[k].n; i++) h[at++] = (uint32_t)lists[k].idx[i];
        SCANRS_HIP(hipMemcpyAsync(d_lists, h, n_all * 4, hipMemcpyHostToDevice, s));
    }
    const uint64_t stride = std::max<uint64_t>(1, n_result);
    unsigned long long *d_out = st.scratch.get<unsigned long long>("subset_out", 2 * stride); // (f64 results take the same 8 bytes)
    const DevMap map = mode == 0 ? DevMap{} : m->dev_map(outer_is_view_row);

    if (!listed_outer) {
        // masked walk over the row copy
        void *d_slab = st.scratch.get<unsigned long long>("subset_slab", 2 * std::max<uint64_t>(1, cp.n_slab));
        if (!per_column) {
            uint8_t *d_code = st.scratch.get<uint8_t>("subset_code", std::max<uint64_t>(1, cp.n_inner));
            SCANRS_HIP(hipMemsetAsync(d_code, 0, std::max<uint64_t>(1, cp.n_inner), s));
            for (int k = 0; k < n_lists; k++) launch_subset_code(st, d_list[k], lists[k].n, (uint8_t)(1u << k), d_code);
            if (cp.n_outer == 0 || cp.n_items == 0) SCANRS_HIP(hipMemsetAsync(d_out, 0, 2 * stride * 8, s));
            subset_progress(snoop, 0.1);
            launch_subset_reduce(st, cp, map, mode, n_lists, d_code, d_out, stride, d_slab);
            subset_progress(snoop, 0.9);
            launch_subset_finish(st, cp, mode, n_out, d_slab, d_out, stride);
        } else {
            // ... with the result per listed column: scattered (u64 only)
            uint32_t *d_pos = st.scratch.get<uint32_t>("subset_pos", std::max<uint64_t>(1, cp.n_inner));
            SCANRS_HIP(hipMemsetAsync(d_pos, 0xFF, std::max<uint64_t>(1, cp.n_inner) * 4, s));
            SCANRS_HIP(hipMemsetAsync(d_out, 0, stride * 8, s));
            launch_subset_pos(st, d_list[0], lists[0].n, d_pos);
            launch_subset_inner_scatter(st, cp, d_pos, d_out);
        }
    } else if (per_column) {
        launch_subset_listed(st, cp, map, mode, d_list[0], lists[0].n, d_out);
    } else {
        // the listed vectors of the column copy, scattered into the rows (u64 only): one walk per list
        SCANRS_HIP(hipMemsetAsync(d_out, 0, 2 * stride * 8, s));
        for (int k = 0; k < n_lists; k++) {
            subset_progress(snoop, n_all ? (double)(k ? lists[0].n : 0) / (double)n_all : 0.0);
            launch_subset_listed_scatter(st, cp, d_list[k], lists[k].n, d_out + (uint64_t)k * stride);
        }
    }
    SCANRS_SYNC(s);
    subset_progress(snoop, 1.0); // (a cancellation up to here leaves the outputs untouched)
    if (n_result)
        for (int k = 0; k < n_out; k++) SCANRS_D2H(out[k], d_out + (uint64_t)k * stride, n_result * 8, s);
    SCANRS_SYNC(s);
    (scatter ? st.subset_scatter_passes : st.subset_masked_passes)++;
}

void sums_one(scanrs_mat *m, bool per_column, int mode, const uint64_t *cols, uint64_t n, void *out) {
    const List l{cols, n, "cols"};
    void *o[2] = {out, nullptr};
    subset_sums(m, per_column, mode, &l, 1, nullptr, o);
}
void sums_dual(scanrs_mat *m, int mode, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2, const scanrs_snoop *snoop,
               void *out1, void *out2) {
    const List l[2] = {{cols1, n1, "cols1"}, {cols2, n2, "cols2"}};
    void *o[2] = {out1, out2};
    subset_sums(m, false, mode, l, 2, snoop, o);
}

} // namespace
} // namespace scanrs

using namespace scanrs;
extern "C" {
int scanrs_mat_sum_rows_u64(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out) {
    return guard([&] { sums_one(m, false, 0, cols, n, out); });
}
int scanrs_mat_sum_rows_f64(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { sums_one(m, false, 1, cols, n, out); });
}
int scanrs_mat_sum_cols_u64(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out) {
    return guard([&] { sums_one(m, true, 0, cols, n, out); });
}
int scanrs_mat_sum_cols_f64(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { sums_one(m, true, 1, cols, n, out); });
}
int scanrs_mat_sum_rows_dual_u64(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                 const scanrs_snoop *snoop, uint64_t *out1, uint64_t *out2) {
    return guard([&] { sums_dual(m, 0, cols1, n1, cols2, n2, snoop, out1, out2); });
}
int scanrs_mat_sum_rows_dual_f64(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                 const scanrs_snoop *snoop, double *out1, double *out2) {
    return guard([&] { sums_dual(m, 1, cols1, n1, cols2, n2, snoop, out1, out2); });
}
int scanrs_mat_mean_rows(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { // sqz/src/mat.rs:279-282
        sums_one(m, false, 1, cols, n, out);
        const double len = (double)n;
        for (uint64_t i = 0, r = m->rows(); i < r; i++) out[i] = out[i] / len; // (an empty list: 0.0 / 0.0, as the reference)
    });
}
int scanrs_mat_mean_var_rows(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *mean, double *var) {
    return guard([&] { // sqz/src/mat.rs:333-374
        const List l{cols, n, "cols"};
        void *o[2] = {mean, var};
        subset_sums(m, false, 2, &l, 1, nullptr, o);
        const double len = (double)n;
        for (uint64_t i = 0, r = m->rows(); i < r; i++) { // V[X] = E[X^2] - E[X]^2 (:366-371)
            mean[i] = mean[i] / len;
            var[i] = var[i] / len - mean[i] * mean[i];
        }
    });
}
} // extern "C"
