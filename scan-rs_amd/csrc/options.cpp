// options.cpp — the keys of scanrs_mat_set_option, scanrs_set_global_option and scanrs_mat_get_counter, one table each, and the
// one parser every option value goes through (the route decode of scanrs_host_spmm_route included). A new option is a member of
// Options (options.hpp) and a row here; a new counter is a member of Storage and a row here; both get a paragraph in scanrs_amd.h.
#include <algorithm>
#include <cmath>
#include <iterator>
#include <type_traits>

#include "common.hpp"

namespace scanrs {
namespace {

enum Kind {
    INT,      // a whole number in [lo, hi]
    ENDS,     // lo or hi, nothing between
    KB,       // a whole number of KB in [lo, hi], stored as bytes
    FLAG,     // nonzero -> 1
    THREEWAY, // 2 -> 2, any other nonzero -> 1, 0 -> 0
    REAL,     // [lo, hi] or (lo, hi], as given
    TRUNC,    // [lo, hi], the fraction dropped
    CLAMP     // raised to lo / lowered to hi, the fraction dropped (global options only)
};
enum : unsigned { OPEN_LO = 1, SETTABLE = 2, GLOBAL = 4 }; // (the first two as scanrs_host_option_info reports them)
struct OptionRow {
    const char *name;
    Kind kind;
    double lo, hi;
    unsigned flags;
    double dflt;
    void (*store)(Options &, double); // a global row ignores the Options
    void (*hook)(Storage &);          // after the store, or nullptr
};
constexpr double INF = HUGE_VAL;
constexpr double U64_SAFE = 9223372036854774784.0; // the largest double below 2^63

template <auto M, class T>
void store_member(T &t, double v) {
    t.*M = static_cast<std::remove_reference_t<decltype(t.*M)>>(v);
}
template <auto M>
void store_global(Options &, double v) {
    store_member<M>(global_options(), v);
}
template <auto M>
OptionRow opt(const char *name, Kind kind, double lo, double hi, unsigned flags = SETTABLE, void (*hook)(Storage &) = nullptr) {
    return {name, kind, lo, hi, flags, (double)(Options().*M) / (kind == KB ? 1024.0 : 1.0), store_member<M, Options>, hook};
}
template <auto M>
OptionRow flag(const char *name, void (*hook)(Storage &) = nullptr) {
    return opt<M>(name, FLAG, 0, 1, SETTABLE, hook);
}
template <auto M>
OptionRow glob(const char *name, Kind kind, double lo, double hi) {
    return {name, kind, lo, hi, SETTABLE | GLOBAL, (double)(GlobalOptions().*M), store_global<M>, nullptr};
}
// deadline of every host-side wait for the device (common.hpp, "bounded waits"): process-wide, a key of both setters
const OptionRow SYNC_TIMEOUT = {"sync_timeout_s", REAL, 0, INF, OPEN_LO | SETTABLE | GLOBAL, 120.0, [](Options &, double v) { set_sync_timeout_s(v); }, nullptr};

void forget_tile_weights(Storage &st) { // (the form of the weights follows tile_wtab and tile_fold)
    tile_layout_forget_weights(st.primary.tiles.get());
    tile_layout_forget_weights(st.other.tiles.get());
}

// The four shape options are usually set one after the other: a combination is checked as a whole when the product runs
// (launch_spmm_tiles / tile_layout_build refuse an unsupported shape); each value alone must be one some shape uses.
const OptionRow HANDLE_OPTIONS[] = {
    opt<&Options::tile_k>("tile_k", INT, 2, 4),
    opt<&Options::tile_s>("tile_s", ENDS, 28, 32),
    opt<&Options::tile_ku>("tile_ku", INT, 0, 1),
    opt<&Options::tile_t>("tile_t", INT, 8, 96),
    opt<&Options::tile_b>("tile_b", INT, 2, 24),
    flag<&Options::dense_side_no_lds>("dense_side_no_lds"),
    opt<&Options::side_build>("side_build", INT, 0, 2),
    flag<&Options::tile_split>("tile_split"),
    opt<&Options::tile_split_x>("tile_split_x", REAL, 0.05, 16, OPEN_LO | SETTABLE),
    opt<&Options::tile_split_min>("tile_split_min", REAL, 0, 16),
    flag<&Options::tile_build_one_pass>("tile_build_one_pass"),
    flag<&Options::tile_weights_wide>("tile_weights_wide"),
    flag<&Options::tile_dense>("tile_dense"),
    opt<&Options::tile_sort_slots>("tile_sort_slots", THREEWAY, 0, 2),
    flag<&Options::tile_wtab>("tile_wtab", forget_tile_weights),
    flag<&Options::tile_fold>("tile_fold", forget_tile_weights),
    opt<&Options::tile_big_list_cap>("tile_big_list_cap", TRUNC, 0, 4.0e9),
    flag<&Options::tile_one_walk>("tile_one_walk"),
    flag<&Options::tile_emit_staged>("tile_emit_staged"),
    flag<&Options::tile_builder>("tile_builder"),
    opt<&Options::tile_build_waves>("tile_build_waves", TRUNC, 0, 32),
    opt<&Options::ov_tile_bytes>("ov_tile_kb", KB, 0, 4194304),
    opt<&Options::tile_max_overflow>("tile_max_overflow", REAL, 0, 1, OPEN_LO | SETTABLE),
    flag<&Options::tile_auto>("tile_auto"),
    flag<&Options::tile_overlap>("tile_overlap"),
    opt<&Options::l2_tile_bytes>("l2_tile_kb", KB, 64, 4194304),
    opt<&Options::spmm_order>("spmm_order", INT, 0, 2),
    flag<&Options::materialize>("materialize"),
    opt<&Options::hot_segment>("hot_segment", INT, 0, 4294967295.0),
    flag<&Options::slice_walk>("slice_walk"),
    flag<&Options::spmv_lds>("spmv_lds"),
    flag<&Options::overlap>("overlap"),
    opt<&Options::col_moments>("col_moments", INT, 0, 2),
    flag<&Options::device_factor>("device_factor"),
    opt<&Options::sseq_grid_cap>("sseq_grid_cap", INT, 1, 16384),
    opt<&Options::merge_fused>("merge_fused", INT, 0, 1),
    opt<&Options::subset_scatter>("subset_scatter", INT, 0, 1),
    opt<&Options::d2h_threads>("d2h_threads", INT, 1, 256),
    SYNC_TIMEOUT,
    flag<&Options::tile_spare_cus>("tile_spare_cus"),
    flag<&Options::tile_poison_slack>("tile_poison_slack"),
    flag<&Options::spmv_row_table>("spmv_row_table"),
    flag<&Options::gemm_direct>("gemm_direct"),
    opt<&Options::reuse_cmax>("reuse_cmax", REAL, 0, INF, OPEN_LO | SETTABLE),
    // read by the route decision, set by scanrs_mat_set_spmm_path / scanrs_mat_set_panel_precision / nothing: no keys of set_option
    opt<&Options::spmm_path>("spmm_path", INT, 0, 3, 0),
    opt<&Options::panel_precision>("panel_precision", INT, 0, 1, 0),
    opt<&Options::blocked_min_nnz>("blocked_min_nnz", INT, 0, U64_SAFE, 0),
};
// Most of these clamp rather than refuse. (The upper clamps are what the stored type holds.)
const OptionRow GLOBAL_OPTIONS[] = {
    glob<&GlobalOptions::h5_threads>("h5_threads", CLAMP, 1, 2147483647.0),
    glob<&GlobalOptions::eig_threads>("eig_threads", CLAMP, 1, 2147483647.0),
    glob<&GlobalOptions::knn_exhaustive>("knn_exhaustive", FLAG, 0, 1),
    glob<&GlobalOptions::knn_filter_min_points>("knn_filter_min_points", CLAMP, 0, U64_SAFE),
    glob<&GlobalOptions::knn_ratio>("knn_ratio", CLAMP, 2, U64_SAFE),
    glob<&GlobalOptions::knn_block_rows>("knn_block_rows", CLAMP, 1, U64_SAFE),
    glob<&GlobalOptions::knn_stats>("knn_stats", FLAG, 0, 1),
    // share of the device's memory that released blocks may occupy while they wait for reuse
    {"device_cache_fraction", REAL, 0, 1, SETTABLE | GLOBAL, 0.5, [](Options &, double v) { device_cache_set_fraction(v); }, nullptr},
    SYNC_TIMEOUT,
};
// the positional order of scanrs_host_spmm_route's `options` array (ABI)
const char *const ROUTE_ORDER[] = {"spmm_path",  "panel_precision", "tile_auto",      "tile_k",     "tile_s",     "tile_t",
                                   "tile_b",     "tile_ku",         "tile_dense",     "tile_builder", "blocked_min_nnz", "slice_walk",
                                   "spmv_lds",   "spmv_row_table",  "spmm_order",     "materialize", "tile_wtab",  "tile_fold"};

template <class Row>
const Row *find_row(const Row *rows, size_t n, const char *key) {
    for (size_t i = 0; i < n; i++)
        if (!strcmp(rows[i].name, key)) return rows + i;
    return nullptr;
}
const OptionRow *option_rows(int scope, size_t &n) {
    if (scope != 0 && scope != 1) fail(SCANRS_ERR_ARGUMENT, "scope must be 0 (per handle) or 1 (global)");
    n = scope ? std::size(GLOBAL_OPTIONS) : std::size(HANDLE_OPTIONS);
    return scope ? GLOBAL_OPTIONS : HANDLE_OPTIONS;
}
const OptionRow &settable_row(int scope, const char *key) {
    size_t n;
    const OptionRow *rows = option_rows(scope, n), *r = find_row(rows, n, key);
    if (!r || !(r->flags & SETTABLE)) fail(SCANRS_ERR_ARGUMENT, scope ? "unknown global option '%s'" : "unknown option '%s'", key);
    return *r;
}

// What the option stores for `value`. Every value arrives as a double: nothing is cast before it is known to be finite and in
// range (a NaN or a negative number through (uint32_t) is undefined behaviour).
double parse(const OptionRow &r, double value) {
    const bool global_flag = r.kind == FLAG && (r.flags & GLOBAL); // (these two have always read NaN as "on")
    if (!std::isfinite(value) && !global_flag) fail(SCANRS_ERR_ARGUMENT, "option '%s': the value must be finite", r.name);
    const bool whole = r.kind == INT || r.kind == ENDS || r.kind == KB;
    const bool in_range = (r.flags & OPEN_LO ? value > r.lo : value >= r.lo) && value <= r.hi;
    switch (r.kind) {
    case FLAG: return value != 0.0 ? 1.0 : 0.0;
    case THREEWAY: return value == 2.0 ? 2.0 : (value != 0.0 ? 1.0 : 0.0);
    case CLAMP: return std::floor(std::min(std::max(value, r.lo), r.hi));
    default: break;
    }
    if (r.kind == ENDS && value != r.lo && value != r.hi) fail(SCANRS_ERR_ARGUMENT, "option '%s' must be %g or %g", r.name, r.lo, r.hi);
    if (whole && (!in_range || value != std::floor(value))) fail(SCANRS_ERR_ARGUMENT, "option '%s' must be an integer in [%g, %g]", r.name, r.lo, r.hi);
    if (!in_range) fail(SCANRS_ERR_ARGUMENT, "option '%s' must be in %c%g, %g]", r.name, r.flags & OPEN_LO ? '(' : '[', r.lo, r.hi);
    return r.kind == KB ? value * 1024.0 : r.kind == TRUNC ? std::floor(value) : value;
}

// ---- counters ---------------------------------------------------------------------------------------------------------------------
struct CounterRow {
    const char *name;
    uint64_t Storage::*field;    // the plain ones
    uint64_t (*read)(Storage &); // the rest
};
uint64_t f64_bits(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}
template <int I>
uint64_t tile_stat(Storage &st) { // both tile layouts of the handle
    st.side_join_if(nullptr, true);
    uint64_t a[3], b[3];
    tile_layout_stats(st.primary.tiles.get(), a);
    tile_layout_stats(st.has_other ? st.other.tiles.get() : nullptr, b);
    return a[I] + b[I];
}
#define SCANRS_COUNTER(name, expr) {name, nullptr, [](Storage &st) -> uint64_t { return expr; }}
const CounterRow COUNTERS[] = {
    {"bk_host_retries", &Storage::bk_host_retries, nullptr},
    // what the last svd_bk on this handle decided about its reused projection (Storage::BkDecisions)
    SCANRS_COUNTER("bk_q", st.bk.q),
    SCANRS_COUNTER("bk_b", st.bk.b),
    SCANRS_COUNTER("bk_coef_valid", st.bk.coef_valid),
    SCANRS_COUNTER("bk_flagged_older", st.bk.flagged_older),
    SCANRS_COUNTER("bk_limit_branch", st.bk.limit_branch),
    SCANRS_COUNTER("bk_limit_bits", f64_bits(st.bk.limit)),
    SCANRS_COUNTER("bk_direct_columns", st.bk.direct_columns),
    SCANRS_COUNTER("bk_last_direct", st.bk.last_direct),
    SCANRS_COUNTER("bk_full_direct", st.bk.full_direct),
    SCANRS_COUNTER("bk_early_projections", st.bk.early_projections),
    SCANRS_COUNTER("bk_cmax_dense_bits", f64_bits(st.bk.cmax_dense)),
    // the last sparse product on this handle (Storage::SpmmDecision): its kernel family, SCANRS_SPMM_*, the form within the family,
    // and its column chunks, SCANRS_SPMM_SLIVER set when a last narrow one went to the plain gather
    SCANRS_COUNTER("spmm_route", st.spmm.family),
    SCANRS_COUNTER("spmm_form", st.spmm.form),
    SCANRS_COUNTER("spmm_chunks", st.spmm.chunks),
    // the sort the handle's transposed copy was built through (transpose_plan.hpp): 0 none built or no nonzeros, 1 packed key,
    // 2 pair sort (a helper thread may be building the copy right now)
    SCANRS_COUNTER("transpose_route", (st.side_join_if(&st.other, false), st.transpose_route)),
    {"partition_rounds", &Storage::partition_rounds, nullptr},
    {"partition_allreduces", &Storage::partition_allreduces, nullptr},
    {"de_pairs_passes", &Storage::de_pairs_passes, nullptr},
    {"de_pairs_literal", &Storage::de_pairs_literal, nullptr},
    {"de_shard_tests", &Storage::de_shard_tests, nullptr},
    {"de_shard_allreduces", &Storage::de_shard_allreduces, nullptr},
    {"subset_masked_passes", &Storage::subset_masked_passes, nullptr},
    {"subset_scatter_passes", &Storage::subset_scatter_passes, nullptr},
    {"knn_blocks", &Storage::knn_blocks, nullptr},
    {"knn_allreduces", &Storage::knn_allreduces, nullptr},
    {"knn_blocks_filtered", &Storage::knn_blocks_filtered, nullptr},
    {"subset_allreduces", &Storage::subset_allreduces, nullptr},
    // wall clock of a shard's phases (multi.cpp): made by an inner-sharding constructor; by scanrs_multi_gather_outer / _rebalance;
    // in the last scanrs_multi_to_adaptive
    SCANRS_COUNTER("reshard_upload_us", st.reshard_us[0]),
    SCANRS_COUNTER("reshard_count_us", st.reshard_us[1]),
    SCANRS_COUNTER("reshard_split_us", st.reshard_us[2]),
    SCANRS_COUNTER("reshard_exchange_us", st.reshard_us[3]),
    SCANRS_COUNTER("reshard_transpose_us", st.reshard_us[4]),
    SCANRS_COUNTER("regather_plan_us", st.regather_us[0]),
    SCANRS_COUNTER("regather_pull_us", st.regather_us[1]),
    SCANRS_COUNTER("regather_finish_us", st.regather_us[2]),
    SCANRS_COUNTER("export_plan_us", st.export_us[0]),
    SCANRS_COUNTER("export_pull_us", st.export_us[1]),
    SCANRS_COUNTER("export_encode_us", st.export_us[2]),
    // first-call accounting, host time of the calling thread
    {"t_layout_us", &Storage::t_layout_us, nullptr},
    {"t_side_wait_us", &Storage::t_side_wait_us, nullptr},
    {"t_start_panel_us", &Storage::t_start_panel_us, nullptr},
    {"t_delivery_us", &Storage::t_delivery_us, nullptr},
    SCANRS_COUNTER("t_alloc_us", ((void)st, device_alloc_us())), // hipMalloc, process-wide
    SCANRS_COUNTER("alloc_calls", ((void)st, device_alloc_calls())),
    {"tile_positions", nullptr, tile_stat<0>},
    {"tile_served_nonzeros", nullptr, tile_stat<1>},
    {"tile_overflow_nonzeros", nullptr, tile_stat<2>},
};
#undef SCANRS_COUNTER

} // namespace

void options_from_route_array(const double *values, Options &o) {
    for (size_t i = 0; i < std::size(ROUTE_ORDER); i++) {
        const OptionRow &r = *find_row(HANDLE_OPTIONS, std::size(HANDLE_OPTIONS), ROUTE_ORDER[i]);
        r.store(o, parse(r, values[i]));
    }
}

} // namespace scanrs

using namespace scanrs;

extern "C" {

int scanrs_set_global_option(const char *key, double value) {
    return guard([&] {
        if (!key) fail(SCANRS_ERR_ARGUMENT, "null key");
        const OptionRow &r = settable_row(1, key);
        Options unused;
        r.store(unused, parse(r, value));
    });
}
int scanrs_mat_set_option(scanrs_mat *m, const char *key, double value) {
    return guard([&] {
        if (!m || !key) fail(SCANRS_ERR_ARGUMENT, "null handle or key");
        const OptionRow &r = settable_row(0, key);
        r.store(m->st->opt, parse(r, value));
        if (r.hook) r.hook(*m->st);
    });
}
int scanrs_mat_set_spmm_path(scanrs_mat *m, int path) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (path < 0 || path > 3)
            fail(SCANRS_ERR_ARGUMENT, "path must be 0 (auto), 1 (plain gather), 2 (L2-blocked gather) or 3 (LDS-staged tiles + gather)");
        m->st->opt.spmm_path = path;
    });
}
int scanrs_mat_set_panel_precision(scanrs_mat *m, int precision) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        if (precision != 0 && precision != 1) fail(SCANRS_ERR_ARGUMENT, "precision must be 0 (f64 panels) or 1 (f32 gather panels)");
        m->st->opt.panel_precision = precision;
    });
}
int scanrs_mat_get_counter(scanrs_mat *m, const char *key, uint64_t *value) {
    return guard([&] {
        if (!m || !key || !value) fail(SCANRS_ERR_ARGUMENT, "null argument");
        const CounterRow *r = find_row(COUNTERS, std::size(COUNTERS), key);
        if (!r) fail(SCANRS_ERR_ARGUMENT, "unknown counter '%s'", key);
        *value = r->read ? r->read(*m->st) : (*m->st).*(r->field);
    });
}

int scanrs_host_option_info(int scope, uint32_t index, const char **name, double *dflt, double *lo, double *hi, uint32_t *flags) {
    return guard([&] {
        if (!name || !dflt || !lo || !hi || !flags) fail(SCANRS_ERR_ARGUMENT, "null argument");
        size_t n;
        const OptionRow *rows = option_rows(scope, n);
        if (index >= n) fail(SCANRS_ERR_ARGUMENT, "no option %u in scope %d", index, scope);
        const OptionRow &r = rows[index];
        *name = r.name, *dflt = r.dflt, *lo = r.lo, *hi = r.hi;
        uint32_t route = 0;
        for (uint32_t i = 0; !scope && i < std::size(ROUTE_ORDER); i++)
            if (!strcmp(ROUTE_ORDER[i], r.name)) route = i + 1;
        *flags = (r.flags & OPEN_LO ? SCANRS_OPTION_OPEN_LO : 0u) | (r.flags & SETTABLE ? SCANRS_OPTION_SETTABLE : 0u) | (route << SCANRS_OPTION_ROUTE_SHIFT);
    });
}
int scanrs_host_option_parse(int scope, const char *name, double value, double *stored) {
    return guard([&] {
        if (!name || !stored) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *stored = parse(settable_row(scope, name), value);
    });
}
int scanrs_host_counter_name(uint32_t index, const char **name) {
    return guard([&] {
        if (!name) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (index >= std::size(COUNTERS)) fail(SCANRS_ERR_ARGUMENT, "no counter %u", index);
        *name = COUNTERS[index].name;
    });
}

} // extern "C"
