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
//
// A sharded handle (the *_sharded entry points, collective) runs the same forms on the rank's own storage with its part of
// the lists, then:
//
//   the result runs along the sharded dimension    every result is owned by one rank: the rank's results go to their place in a
//   (sum_rows* with sharded rows, sum_cols with    zero-filled array of the whole extent, one u64 all-reduce of the bit patterns
//   sharded columns)                               copies them to everyone (1 exchange step)
//   the sum crosses the shards, u64                the partial sums are added by one u64 all-reduce (1 step)
//   the sum crosses the shards, f64                the fixed-point form of the walk (subset.hip): a pre-pass finds the largest |term|,
//                                                  slot r of a world-long array carries rank r's (step 1), every rank derives the same
//                                                  quantum, the 128-bit sums cross as 32-bit limbs (step 2), the host converts
#include "common.hpp"
#include "fixed128.hpp"
#include "shard_exchange.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace scanrs {

namespace {

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

// The quantum of a fixed-point sum (scanrs_amd.h states the rule): fixed_scale of bound = largest |term| x largest number of terms, so
// that every sum stays below 2^124. A bound that is not finite has no quantum: the NaN makes the kernels flag every term. (Bounds
// below 2^-877 keep the scale itself finite.)
double fx_scale(double bound) {
    if (!std::isfinite(bound)) return NAN;
    if (bound > 0.0 && std::ilogb(bound) < -877) return std::ldexp(1.0, 1000);
    return fixed_scale(bound);
}

// the extent of the view's rows over all shards
uint64_t rows_all(const scanrs_mat *m) { return rows_sharded(m) ? m->st->shard.outer_global : m->rows(); }

// per_column false: out[k] (rows entries) = sums of every row over list k. per_column true (one list): out[0] (n entries) = the sums
// of the listed columns over all rows. mode 0: u64 of the raw counts; 1: f64 of the mapped values; 2: out[0] = sums, out[1] = sums of
// squares of the mapped values over the one list. collective: the call of a *_sharded entry point (a sharded handle is served; lists
// and results along the sharded dimension span the whole matrix).
void subset_sums(scanrs_mat *m, bool per_column, int mode, const List *lists, int n_lists, const scanrs_snoop *snoop, void *const *out,
                 bool collective) {
    if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
    Storage &st = *m->st;
    const bool sharded = st.shard.active();
    const bool list_global = sharded && cols_sharded(m);                                       // the lists name the sharded dimension
    const bool result_global = sharded && (per_column ? cols_sharded(m) : rows_sharded(m)); // every result is owned by one rank
    const bool crossing = sharded && !result_global;                                        // every result is a sum over all ranks
    const uint64_t rows = m->rows(), cols = m->cols();                                      // (the rank's own)
    const uint64_t cols_g = list_global ? st.shard.outer_global : cols, rows_g = rows_all(m);
    const uint64_t n_final = per_column ? lists[0].n : rows_g; // entries of every output
    const int n_out = mode == 2 ? 2 : n_lists;
    for (int k = 0; k < n_out; k++)
        if (n_final && !out[k]) fail(SCANRS_ERR_ARGUMENT, "null argument");
    if (sharded && !collective) fail(SCANRS_ERR_ARGUMENT, "sums over a column list of a sharded handle are not supported");
    if (collective) st.subset_allreduces = 0;
    if (mode == 0 && !map_is_raw(m)) fail(SCANRS_ERR_ARGUMENT, "u64 sums are defined on the raw count matrix");
    uint64_t n_terms = per_column ? rows_g : 0; // the most terms a result can have (the fixed-point quantum)
    for (int k = 0; k < n_lists; k++) {
        check_list(lists[k].idx, lists[k].n, cols_g, lists[k].name);
        if (!per_column) n_terms = std::max(n_terms, lists[k].n);
    }
    // the rank's part of a list along the sharded dimension, in local positions; `below`: the entries that lie on lower ranks
    List local[2] = {lists[0], lists[n_lists > 1 ? 1 : 0]};
    std::vector<uint64_t> rebased[2];
    uint64_t below = 0;
    if (list_global)
        for (int k = 0; k < n_lists; k++) {
            const uint64_t lo = st.shard.outer_begin, hi = lo + cols;
            const uint64_t *first = std::lower_bound(lists[k].idx, lists[k].idx + lists[k].n, lo);
            const uint64_t *last = std::lower_bound(first, lists[k].idx + lists[k].n, hi);
            rebased[k].assign(first, last);
            for (uint64_t &x : rebased[k]) x -= lo;
            if (k == 0) below = (uint64_t)(first - lists[k].idx);
            local[k].idx = rebased[k].data();
            local[k].n = rebased[k].size();
        }
    const uint64_t n_result = per_column ? local[0].n : rows; // results this rank computes
    uint64_t n_all = 0;
    for (int k = 0; k < n_lists; k++) n_all += local[k].n;
    snoop_poll(snoop, 0.0); // (a flag that is already set: nothing has been queued, the outputs are untouched)

    CurrentHandle cur(&st);
    hipStream_t s = st.stream;
    ShardExchange ex{st, st.subset_allreduces};
    // the copy whose outer dimension is the result axis: does it exist? (other_settled, not has_other: the route must not depend on
    // how far a helper thread has come)
    const bool want_base_rows = (!per_column) != m->transposed;
    const bool exists = want_base_rows == (st.storage == SCANRS_CSR) || st.other_settled;
    const bool scatter = !exists && mode == 0 && st.opt.subset_scatter != 0;
    SparseCopy &cp = scatter ? st.primary : st.copy_with_outer_rows(want_base_rows);
    const bool outer_is_view_row = scatter ? per_column : !per_column;
    const bool listed_outer = !outer_is_view_row; // the lists name view columns
    const bool fixed = crossing && mode != 0 && n_final != 0; // (mode != 0 never scatters: the walk below is the masked one or the listed one)

    // the lists, narrowed to u32, through the pinned staging buffer
    uint32_t *d_lists = st.scratch.get<uint32_t>("subset_lists", std::max<uint64_t>(1, n_all));
    const uint32_t *d_list[2] = {d_lists, d_lists + local[0].n};
    if (n_all) {
        uint32_t *h = static_cast<uint32_t *>(st.pinned(n_all * 4));
        uint64_t at = 0;
        for (int k = 0; k < n_lists; k++)
            for (uint64_t i = 0; i < local[k].n; i++) h[at++] = (uint32_t)local[k].idx[i];
        SCANRS_HIP(hipMemcpyAsync(d_lists, h, n_all * 4, hipMemcpyHostToDevice, s));
    }
    const uint64_t stride = std::max<uint64_t>(1, n_result);
    unsigned long long *d_out = st.scratch.get<unsigned long long>("subset_out", 2 * stride); // (f64 results take the same 8 bytes)
    const DevMap map = mode == 0 ? DevMap{} : m->dev_map(outer_is_view_row);

    // the fixed-point form: 4 words and a flag per result, and the quantum all ranks agree on
    unsigned long long *d_fx = nullptr;
    uint32_t *d_bad = nullptr;
    double scale[2] = {1.0, 1.0};
    auto agree_on_scales = [&](unsigned long long *d_max) {
        // every rank's largest |term|: the maximum of the bit patterns is the maximum of the values
        const std::vector<unsigned long long> h = ex.gather(d_max, 1);
        const unsigned long long bits = *std::max_element(h.begin(), h.end());
        double mx;
        memcpy(&mx, &bits, 8);
        scale[0] = fx_scale(mx * (double)n_terms);
        scale[1] = mode == 2 ? fx_scale(mx * mx * (double)n_terms) : scale[0];
    };
    unsigned long long *d_max = nullptr;
    if (fixed) {
        d_fx = st.scratch.get<unsigned long long>("subset_fx", 4 * stride);
        d_bad = st.scratch.get<uint32_t>("subset_fx_bad", stride);
        d_max = st.scratch.get<unsigned long long>("subset_max", 1);
        SCANRS_HIP(hipMemsetAsync(d_max, 0, 8, s));
    }

    if (!listed_outer) {
        // masked walk over the row copy
        if (!per_column) {
            uint8_t *d_code = st.scratch.get<uint8_t>("subset_code", std::max<uint64_t>(1, cp.n_inner));
            SCANRS_HIP(hipMemsetAsync(d_code, 0, std::max<uint64_t>(1, cp.n_inner), s));
            for (int k = 0; k < n_lists; k++) launch_subset_code(st, d_list[k], local[k].n, (uint8_t)(1u << k), d_code);
            if (fixed) {
                unsigned long long *d_slab = st.scratch.get<unsigned long long>("subset_slab_fx", 5 * std::max<uint64_t>(1, cp.n_slab));
                launch_subset_reduce_max(st, cp, map, d_code, d_max);
                agree_on_scales(d_max);
                snoop_poll(snoop, 0.1);
                launch_subset_reduce_fx(st, cp, map, mode, n_lists, d_code, scale[0], scale[1], d_fx, d_bad, d_slab);
                snoop_poll(snoop, 0.9);
            } else {
                void *d_slab = st.scratch.get<unsigned long long>("subset_slab", 2 * std::max<uint64_t>(1, cp.n_slab));
                if (cp.n_outer == 0 || cp.n_items == 0) SCANRS_HIP(hipMemsetAsync(d_out, 0, 2 * stride * 8, s));
                snoop_poll(snoop, 0.1);
                launch_subset_reduce(st, cp, map, mode, n_lists, d_code, d_out, stride, d_slab);
                snoop_poll(snoop, 0.9);
                launch_subset_finish(st, cp, mode, n_out, d_slab, d_out, stride);
            }
        } else {
            // ... with the result per listed column: scattered (u64 only)
            uint32_t *d_pos = st.scratch.get<uint32_t>("subset_pos", std::max<uint64_t>(1, cp.n_inner));
            SCANRS_HIP(hipMemsetAsync(d_pos, 0xFF, std::max<uint64_t>(1, cp.n_inner) * 4, s));
            SCANRS_HIP(hipMemsetAsync(d_out, 0, stride * 8, s));
            launch_subset_pos(st, d_list[0], local[0].n, d_pos);
            launch_subset_inner_scatter(st, cp, d_pos, d_out);
        }
    } else if (per_column) {
        if (fixed) {
            launch_subset_listed_max(st, cp, map, d_list[0], local[0].n, d_max);
            agree_on_scales(d_max);
            launch_subset_listed_fx(st, cp, map, d_list[0], local[0].n, scale[0], d_fx, d_bad);
        } else {
            launch_subset_listed(st, cp, map, mode, d_list[0], local[0].n, d_out);
        }
    } else {
        // the listed vectors of the column copy, scattered into the rows (u64 only): one walk per list
        SCANRS_HIP(hipMemsetAsync(d_out, 0, 2 * stride * 8, s));
        for (int k = 0; k < n_lists; k++) {
            snoop_poll(snoop, n_all ? (double)(k ? local[0].n : 0) / (double)n_all : 0.0);
            launch_subset_listed_scatter(st, cp, d_list[k], local[k].n, d_out + (uint64_t)k * stride);
        }
    }

    // across the shards
    const unsigned long long *d_res = d_out; // the finished results, k * res_stride + position
    uint64_t res_stride = stride;
    const int n_sums = mode == 2 || n_lists == 2 ? 2 : 1;
    if (fixed) {
        unsigned long long *d_limbs = st.scratch.get<unsigned long long>("subset_limbs", n_final * 5 * n_sums);
        launch_subset_fx_split(st, d_fx, d_bad, n_final, n_sums, d_limbs);
        ex.sum(d_limbs, n_final * 5 * n_sums);
        launch_subset_fx_join(st, d_limbs, n_final, n_sums, d_fx, d_bad);
    } else if (crossing && n_final) {
        ex.sum(d_out, (uint64_t)(n_out - 1) * stride + n_result); // exact partial sums
    } else if (result_global && n_final) {
        // one contributor per element: the sum of the bit patterns is a copy
        const uint64_t at = per_column ? below : st.shard.outer_begin;
        unsigned long long *d_all = st.scratch.get<unsigned long long>("subset_all", (uint64_t)n_out * n_final);
        SCANRS_HIP(hipMemsetAsync(d_all, 0, (uint64_t)n_out * n_final * 8, s));
        if (n_result)
            for (int k = 0; k < n_out; k++)
                SCANRS_HIP(hipMemcpyAsync(d_all + (uint64_t)k * n_final + at, d_out + (uint64_t)k * stride, n_result * 8, hipMemcpyDeviceToDevice, s));
        ex.sum(d_all, (uint64_t)n_out * n_final);
        d_res = d_all;
        res_stride = n_final;
    }
    SCANRS_SYNC(s);
    snoop_poll(snoop, 1.0); // (a cancellation up to here leaves the outputs untouched)
    if (fixed) {
        std::vector<unsigned long long> h_fx(4 * n_final);
        std::vector<uint32_t> h_bad(n_final);
        SCANRS_D2H(h_fx.data(), d_fx, n_final * 32, s);
        SCANRS_D2H(h_bad.data(), d_bad, n_final * 4, s);
        SCANRS_SYNC(s);
        for (int k = 0; k < n_out; k++) {
            double *o = static_cast<double *>(out[k]);
            for (uint64_t i = 0; i < n_final; i++) o[i] = (h_bad[i] >> k) & 1u ? (double)NAN : from_fixed_signed(&h_fx[4 * i + 2 * k], scale[k]);
        }
    } else if (n_final) {
        for (int k = 0; k < n_out; k++) SCANRS_D2H(out[k], d_res + (uint64_t)k * res_stride, n_final * 8, s);
        SCANRS_SYNC(s);
    }
    (scatter ? st.subset_scatter_passes : st.subset_masked_passes)++;
}

void sums_one(scanrs_mat *m, bool per_column, int mode, const uint64_t *cols, uint64_t n, void *out, bool collective) {
    const List l{cols, n, "cols"};
    void *o[2] = {out, nullptr};
    subset_sums(m, per_column, mode, &l, 1, nullptr, o, collective);
}
void sums_dual(scanrs_mat *m, int mode, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2, const scanrs_snoop *snoop,
               void *out1, void *out2, bool collective) {
    const List l[2] = {{cols1, n1, "cols1"}, {cols2, n2, "cols2"}};
    void *o[2] = {out1, out2};
    subset_sums(m, false, mode, l, 2, snoop, o, collective);
}
void mean_rows(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out, bool collective) {
    // sqz/src/mat.rs:279-282
    sums_one(m, false, 1, cols, n, out, collective);
    const double len = (double)n;
    for (uint64_t i = 0, r = rows_all(m); i < r; i++) out[i] = out[i] / len; // (an empty list: 0.0 / 0.0, as the reference)
}
void mean_var_rows(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *mean, double *var, bool collective) {
    // sqz/src/mat.rs:333-374
    const List l{cols, n, "cols"};
    void *o[2] = {mean, var};
    subset_sums(m, false, 2, &l, 1, nullptr, o, collective);
    const double len = (double)n;
    for (uint64_t i = 0, r = rows_all(m); i < r; i++) { // V[X] = E[X^2] - E[X]^2 (:366-371)
        mean[i] = mean[i] / len;
        var[i] = var[i] / len - mean[i] * mean[i];
    }
}

} // namespace
} // namespace scanrs

using namespace scanrs;
extern "C" {
int scanrs_mat_sum_rows_u64(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out) {
    return guard([&] { sums_one(m, false, 0, cols, n, out, false); });
}
int scanrs_mat_sum_rows_f64(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { sums_one(m, false, 1, cols, n, out, false); });
}
int scanrs_mat_sum_cols_u64(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out) {
    return guard([&] { sums_one(m, true, 0, cols, n, out, false); });
}
int scanrs_mat_sum_cols_f64(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { sums_one(m, true, 1, cols, n, out, false); });
}
int scanrs_mat_sum_rows_dual_u64(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                 const scanrs_snoop *snoop, uint64_t *out1, uint64_t *out2) {
    return guard([&] { sums_dual(m, 0, cols1, n1, cols2, n2, snoop, out1, out2, false); });
}
int scanrs_mat_sum_rows_dual_f64(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                 const scanrs_snoop *snoop, double *out1, double *out2) {
    return guard([&] { sums_dual(m, 1, cols1, n1, cols2, n2, snoop, out1, out2, false); });
}
int scanrs_mat_mean_rows(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { mean_rows(m, cols, n, out, false); });
}
int scanrs_mat_mean_var_rows(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *mean, double *var) {
    return guard([&] { mean_var_rows(m, cols, n, mean, var, false); });
}

// the collective forms (a sharded handle is served; an unsharded one takes the plain path)
int scanrs_mat_sum_rows_u64_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out) {
    return guard([&] { sums_one(m, false, 0, cols, n, out, true); });
}
int scanrs_mat_sum_rows_f64_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { sums_one(m, false, 1, cols, n, out, true); });
}
int scanrs_mat_sum_cols_u64_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out) {
    return guard([&] { sums_one(m, true, 0, cols, n, out, true); });
}
int scanrs_mat_sum_cols_f64_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { sums_one(m, true, 1, cols, n, out, true); });
}
int scanrs_mat_sum_rows_dual_u64_sharded(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                         const scanrs_snoop *snoop, uint64_t *out1, uint64_t *out2) {
    return guard([&] { sums_dual(m, 0, cols1, n1, cols2, n2, snoop, out1, out2, true); });
}
int scanrs_mat_sum_rows_dual_f64_sharded(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                         const scanrs_snoop *snoop, double *out1, double *out2) {
    return guard([&] { sums_dual(m, 1, cols1, n1, cols2, n2, snoop, out1, out2, true); });
}
int scanrs_mat_mean_rows_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out) {
    return guard([&] { mean_rows(m, cols, n, out, true); });
}
int scanrs_mat_mean_var_rows_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *mean, double *var) {
    return guard([&] { mean_var_rows(m, cols, n, mean, var, true); });
}
} // extern "C"
