// spmm_route.hpp — which kernel a sparse product A X runs through, and in which form: host code only, no launch, no device call.
// launch_spmm_f64 (kernels.hip) asks spmm_route() and switches on the answer; the tile layout's weight builders (tiles.hip,
// tiles_dense.inc) set the layout's form from tile_form(); every other place that has to know "will this go through the tile
// kernel?" is written in the predicates below, with its own extra terms beside them. scanrs_host_spmm_route exposes the
// pure part to the CPU test-suite, Storage::SpmmDecision keeps the answer of the last product ("route decision").
#pragma once
#include "common.hpp"

namespace scanrs {

// ---- the thresholds of the routes, each named once ----------------------------------------------------------------------------
constexpr uint32_t TL_LMAX = 104;                    // widest panel of the tile kernel: 192 ring rows x 104 x 8 B = 159744 B of LDS
constexpr uint32_t TL_LMIN = 16;                     // ... and the narrowest
constexpr uint32_t TL_LDS = 160u << 10;
constexpr uint64_t TILE_AUTO_MIN_NNZ = 1ull << 24;   // auto path: smaller matrices are not worth a tile layout
constexpr uint64_t FAR_INNER_MIN = 1ull << 19;       // Ix1 / Ix2: an inner-indexed vector of this many positions no longer fits an XCD's L2 (slice_walk, spmv2d, the row reductions)
constexpr uint64_t SPMV_LDS_MIN_OUTER = 1ull << 16;  // spmv_lds: many outer vectors ...
constexpr uint64_t SPMV_LDS_PART = 18432;            // ... against a vector staged in LDS parts of this many positions,
constexpr uint64_t SPMV_LDS_MIN_INNER = 8192;        // ... 64 KB
constexpr uint64_t SPMV_LDS_MAX_INNER = 8 * SPMV_LDS_PART; // ... to 1.1 MB
constexpr uint64_t ORDERED_MAX_OUTER = 65536;        // spmm_order 1: longest-first launch order only for this many outer vectors
// dense tile layout: the kernel's weight tables (tiles_dense.inc)
constexpr uint32_t DN_T = 48, DN_B = 4;              // tile rows, ring buffers
constexpr uint32_t DN_CMAX = 15;                     // largest count that owns a record: the kernel takes a position's weight from a table of 16 entries by count (0: null record); larger counts live in the overflow part
constexpr uint32_t DN_TABK = DN_CMAX + 1u;           // entries per place / planes of the kernel's weight tables
constexpr uint32_t DN_TABI_FRONT = DN_B * DN_T, DN_TABI_PAD = 512; // inner-side table: entries in front of plane 0 (a record of another round may point one ring turn back) and behind every plane (the visits past a part's end)

// ---- the question ---------------------------------------------------------------------------------------------------------------
struct SpmmQuery {
    Options o;
    uint64_t n_outer = 0, n_inner = 0, nnz = 0; // of the copy
    uint32_t l = 0, ldx = 0;
    int n_links = 0; // the map: kind and "indexes its array by the outer position" per link
    int kind[MAX_OPS] = {}, a_outer[MAX_OPS] = {};
    // The one input that is not a number of the question: materialized map values exist for this copy or the device has room for
    // them. launch_spmm_f64 asks the driver only when the route decided with `true` would materialize (fvals_room, kernels.hip).
    bool values_room = true;
};
inline SpmmQuery spmm_query(const Storage &st, const SparseCopy &cp, const DevMap &map, uint32_t l, uint32_t ldx) {
    SpmmQuery q;
    q.o = st.opt;
    q.n_outer = cp.n_outer, q.n_inner = cp.n_inner, q.nnz = cp.nnz;
    q.l = l, q.ldx = ldx;
    q.n_links = map.n;
    for (int i = 0; i < map.n; i++) q.kind[i] = map.ops[i].kind, q.a_outer[i] = map.ops[i].a_outer;
    return q;
}

// ---- the answer -----------------------------------------------------------------------------------------------------------------
// (the values of SCANRS_SPMM_* in scanrs_amd.h)
enum SpmmFamily { SPMM_NONE = 0, SPMM_TILES = 1, SPMM_GATHER2D = 2, SPMM_GATHER2D_F32 = 3, SPMM_SLICE_WALK = 4, SPMM_SPMV2D = 5, SPMM_SPMV_LDS = 6, SPMM_SPMV = 7, SPMM_GATHER = 8 };
// form of a tile product, the fields of TileLayout that tile_layout_weights / dense_layout_weights set
struct TileForm {
    bool dense = false, unit_mode = false, separable = false;
    int nl_outer = 1;  // a separable map: the side that owns the nonlinear links
    int wsrc = 0;      // dense: a position's weight from 0 the stream, 1 the table by (place, count), 2 the table by (count, inner position)
    bool fold_inner = false, fold_outer = false;
};
struct SpmmRoute {
    SpmmFamily family = SPMM_NONE;
    // spmv_lds: VM 0 (the map per nonzero) / 1 (materialized values) / 2 (row table)
    int vm = 0;
    // slice_walk, spmv_lds: materialized values of the first `fstart` links are read; slice_walk: the first link's inner-indexed
    // scale is staged beside the vector (lazy); spmv2d: that scale is interleaved with the vector (fused)
    bool materialized = false, lazy_scale = false, fused = false;
    int fstart = 0;
    TileForm tile; // tiles
    // tiles: column chunks of equal width; a last chunk narrower than the tile kernel takes goes to the plain gather (sliver)
    uint32_t chunks = 1, chunk_width = 0;
    bool sliver = false;
    bool even_ld = false; // the family fails panels whose leading dimensions are odd
    // packed for the counters "spmm_form" / "spmm_chunks" (documented in scanrs_amd.h)
    uint64_t form_bits() const {
        switch (family) {
        case SPMM_TILES: return (tile.dense ? 1u : 0u) | (tile.unit_mode ? 2u : 0u) | ((uint64_t)tile.wsrc << 2) | ((tile.fold_inner ? 1u : tile.fold_outer ? 2u : 0u) << 4);
        case SPMM_SPMV_LDS: return (uint64_t)vm;
        case SPMM_SLICE_WALK:
        case SPMM_SPMV2D: return (materialized ? 1u : 0u) | (fused ? 2u : 0u) | (lazy_scale ? 4u : 0u);
        default: return 0;
        }
    }
    uint64_t chunk_bits() const { return chunks | (sliver ? 1ull << 16 : 0ull); }
};

// ---- predicates, each written once ----------------------------------------------------------------------------------------------
inline bool path_plain_gather(const Options &o) { return o.spmm_path == 1; }
inline bool path_auto(const Options &o) { return o.spmm_path == 0; }
inline bool path_forces_tiles(const Options &o) { return o.spmm_path == 3; }
inline bool path_forces_blocked(const Options &o) { return o.spmm_path == 2 || o.spmm_path == 3; }
inline bool f64_panels(const Options &o) { return o.panel_precision == 0; }
// unit positions exist for K = 2 only (one unit + one general position per visit)
inline bool tile_shape_ok(uint32_t K, uint32_t S, uint32_t T, uint32_t B) {
    const bool ks = (K == 2 && (S == 32 || S == 28)) || (K == 3 && S == 32) || (K == 4 && (S == 32 || S == 28));
    return ks && B >= 2 && T >= 8 && T <= 24u * K && B * T <= 192;
}
inline bool tile_shape_ok(const Options &o) { return tile_shape_ok(o.tile_k, o.tile_s, o.tile_t, o.tile_b); }
// the default shape with the wave-level builder: what the dense record layout serves and what the slot split is made for
inline bool default_tile_shape(const Options &o) { return o.tile_builder != 0 && o.tile_k == 2u && o.tile_b == 4u && o.tile_s == 32u && o.tile_t == 48u; }
inline bool tile_dense_wanted(const Options &o) { return o.tile_dense != 0 && default_tile_shape(o); }
inline uint32_t tile_unit_positions(const Options &o) { return o.tile_k == 2u && o.tile_ku ? 1u : 0u; }
inline bool tile_auto_size(const Options &o, uint64_t nnz) { return nnz >= std::max<uint64_t>(o.blocked_min_nnz, TILE_AUTO_MIN_NNZ); }
// the tile kernel's 32-bit visit index
inline bool tile_visits_fit(const Options &o, uint64_t n_outer, uint64_t n_inner) {
    return ((n_outer + o.tile_s - 1) / o.tile_s) * ((n_inner + o.tile_t - 1) / o.tile_t) <= 0xFFFFFFFFull;
}
// the auto path's own terms for a copy (no panel): what tile_layout_build_auto and spmm_tiles_auto test before they look at the
// layout, the rejection memory and the free memory. Neither the path nor the panel precision: the callers have tested them.
inline bool tile_auto_copy_ok(const Options &o, uint64_t n_outer, uint64_t n_inner, uint64_t nnz) {
    return o.tile_auto && tile_auto_size(o, nnz) && tile_shape_ok(o) && tile_visits_fit(o, n_outer, n_inner);
}
// wide panels go through the tile kernel in column chunks of equal, even width (200 -> 2 x 100, 500 -> 5 x 100)
inline uint32_t tile_chunks(uint32_t l) { return (l + TL_LMAX - 1u) / TL_LMAX; }
inline uint32_t tile_chunk_width(uint32_t l) { return l ? even_up((l + tile_chunks(l) - 1u) / tile_chunks(l)) : 0u; }
// a panel of l columns (one chunk) and this copy fit the tile kernel
inline bool tile_panel_ok(const Options &o, uint64_t n_outer, uint64_t n_inner, uint64_t nnz, uint32_t ldx, uint32_t l) {
    return l >= TL_LMIN && l <= TL_LMAX && (ldx & 1u) == 0 && n_outer > 0 && n_inner > 0 && nnz > 0 &&
           ((size_t)o.tile_b * o.tile_t + 1u) * even_up(l) * 8 <= TL_LDS && (size_t)o.tile_t * even_up(l) * 8 >= 1024u; // (a tile is at least one staging chunk)
}
// Could the product of this query run through the tile kernel? Everything that needs neither the layout nor free memory; on the
// auto path the layout has to exist or be built besides (spmm_tiles_auto), a forced path builds it whatever the overflow.
// A forced path 3 ignores the panel precision.
inline bool tiles_static_candidate(const SpmmQuery &q) {
    const uint32_t lc = tile_chunk_width(q.l);
    if (!(q.l >= TL_LMIN && lc >= TL_LMIN && tile_panel_ok(q.o, q.n_outer, q.n_inner, q.nnz, q.ldx, std::min(lc, q.l)) && tile_shape_ok(q.o))) return false;
    return path_forces_tiles(q.o) || (path_auto(q.o) && f64_panels(q.o) && tile_auto_copy_ok(q.o, q.n_outer, q.n_inner, q.nnz));
}
// L2-blocked gather and spmv2d: outer vectors launched longest first
inline bool launch_longest_first(const Options &o, uint64_t n_outer) { return o.spmm_order == 2 || (o.spmm_order == 1 && n_outer <= ORDERED_MAX_OUTER); }
// the row reductions and the Ix1 / Ix2 products walk an inner-indexed array in slices from here on
inline bool far_inner(const Options &o, uint64_t n_inner, uint64_t nnz) { return nnz >= o.blocked_min_nnz && n_inner >= FAR_INNER_MIN; }

// ---- the map, as the decision reads it --------------------------------------------------------------------------------------------
inline bool link_nonlinear(int k) { return k == OP_LN_1P || k == OP_LOG2_1P || k == OP_LOG10_1P || k == OP_SQUARE; }
inline bool link_binomial(int k) { return k == OP_BINOM_DEV || k == OP_BINOM_PEARSON; }
// does the link read an array by the inner position? (a ScaleAxis holds `a`, a binomial link `a` and `b` on opposite sides)
inline bool link_reads_inner(const SpmmQuery &q, int i) { return (q.kind[i] == OP_SCALE_AXIS && !q.a_outer[i]) || link_binomial(q.kind[i]); }
// everything up to the trailing run of outer-indexed ScaleAxis links: the prefix whose values are worth keeping per nonzero
inline int values_prefix_len(const SpmmQuery &q) {
    int n = q.n_links;
    while (n > 0 && q.kind[n - 1] == OP_SCALE_AXIS && q.a_outer[n - 1]) n--;
    return n;
}
// keep the first n links' values per nonzero? For the gather's sake: few long outer vectors and an inner-indexed link among them
inline bool values_wanted(const SpmmQuery &q, int n) {
    if (!q.o.materialize || n <= 0 || n > MAX_OPS || q.n_outer >= q.n_inner || q.nnz < q.o.blocked_min_nnz) return false;
    bool inner_indexed = false;
    for (int i = 0; i < n; i++) inner_indexed = inner_indexed || link_reads_inner(q, i);
    return inner_indexed && q.values_room;
}
// ... for the arithmetic's sake, on a copy of any shape: a logarithm or a residual link in a product that runs many times
inline bool values_wanted_for_alu(const SpmmQuery &q, int n) {
    if (!q.o.materialize || n <= 0 || n > MAX_OPS || q.nnz < q.o.blocked_min_nnz) return false;
    bool heavy = false;
    for (int i = 0; i < n; i++) heavy = heavy || q.kind[i] == OP_LN_1P || q.kind[i] == OP_LOG2_1P || q.kind[i] == OP_LOG10_1P || link_binomial(q.kind[i]);
    return heavy && q.values_room;
}
// chain shapes the slice walk evaluates from link `from` on: no inner-indexed link at all, or exactly one — a ScaleAxis in first position
inline bool slice_walk_chain(const SpmmQuery &q, int from, bool &lazy_scale) {
    lazy_scale = false;
    for (int i = from; i < q.n_links; i++) {
        if (!link_reads_inner(q, i)) continue;
        if (i == 0 && from == 0 && q.kind[0] == OP_SCALE_AXIS && !q.a_outer[0])
            lazy_scale = true;
        else
            return false;
    }
    return true;
}
// Is f(1, outer, inner) a product of an outer and an inner factor? Yes when the links in front of the first nonlinear link
// (log, square) index one side only and no binomial residual link takes part; nl_outer = the side that owns them.
inline bool tile_map_separable(const SpmmQuery &q, int &nl_outer) {
    bool nonlinear = false, pre_outer = false, pre_inner = false, post_scale = false;
    for (int i = 0; i < q.n_links; i++) {
        const int k = q.kind[i];
        if (link_binomial(k)) return false;
        if (link_nonlinear(k)) {
            if (post_scale) return false; // a scale between two nonlinear links does not factor out of the second one
            nonlinear = true;
        }
        if (k == OP_SCALE_AXIS) {
            if (!nonlinear)
                (q.a_outer[i] ? pre_outer : pre_inner) = true;
            else
                post_scale = true;
        }
    }
    if (nonlinear && pre_outer && pre_inner) return false;
    nl_outer = pre_inner ? 0 : 1;
    return true;
}

// ---- the form of a tile product ---------------------------------------------------------------------------------------------------
// dense / unit_positions: of the layout (a layout that structure_matches() the options has tile_dense_wanted / tile_unit_positions)
inline uint64_t dense_tabi_stride(uint64_t n_inner) { return (n_inner + DN_TABI_PAD + 1u) & ~1ull; }
inline TileForm tile_form(const SpmmQuery &q, bool dense, bool unit_positions) {
    TileForm f;
    f.dense = dense;
    f.separable = tile_map_separable(q, f.nl_outer);
    if (!dense) {
        f.unit_mode = unit_positions && f.separable; // a layout with unit positions under a map that does not separate runs the weighted kernel
        return f;
    }
    const bool fold = f.separable && q.o.tile_fold != 0;
    f.fold_inner = fold && f.nl_outer != 0; // the inner side's factor vi rides in the staged panel
    f.fold_outer = fold && f.nl_outer == 0; // the outer side's factor uo is applied by tile_finish_kernel
    // Under a folded separable map the product kernel evaluates the map itself — a table gather by the record's own count and place /
    // inner position — and no per-position weight exists. The stream form remains for maps that do not separate (GLM-PCA residuals),
    // for tile_fold 0 / tile_wtab 0 and for inner-side tables beyond the kernel's 32-bit byte offsets (4 GB).
    const bool tab_ok = fold && q.o.tile_wtab != 0 && (f.nl_outer != 0 || (DN_TABI_FRONT + (uint64_t)DN_TABK * dense_tabi_stride(q.n_inner)) * 8u < 0xFFFF0000ull);
    f.wsrc = tab_ok ? (f.nl_outer ? 1 : 2) : 0;
    return f;
}

// ---- the routes ---------------------------------------------------------------------------------------------------------------------
inline SpmmRoute tile_route(const SpmmQuery &q) {
    SpmmRoute r;
    r.family = SPMM_TILES;
    r.even_ld = true;
    r.chunks = tile_chunks(q.l);
    r.chunk_width = tile_chunk_width(q.l);
    r.sliver = q.l - (r.chunks - 1u) * r.chunk_width < TL_LMIN;
    r.tile = tile_form(q, tile_dense_wanted(q.o), tile_unit_positions(q.o) != 0);
    return r;
}
// everything below the tile attempt
inline SpmmRoute route_below_tiles(const SpmmQuery &q) {
    const Options &o = q.o;
    SpmmRoute r;
    const bool want_2d = path_forces_blocked(o) || (path_auto(o) && q.nnz >= o.blocked_min_nnz && q.l >= TL_LMIN);
    if (want_2d && q.l > 0 && q.n_outer > 0 && q.n_inner > 0) {
        r.family = f64_panels(o) ? SPMM_GATHER2D : SPMM_GATHER2D_F32; // (panel_precision 1: an f32 copy of the panel)
        r.even_ld = f64_panels(o);
        return r;
    }
    if (!(q.l <= 2 && q.l > 0 && q.n_outer > 0)) {
        r.family = SPMM_GATHER;
        return r;
    }
    r.even_ld = true;
    const bool long_outer = q.n_outer >= q.n_inner;
    const bool far = !path_plain_gather(o) && far_inner(o, q.n_inner, q.nnz);
    r.fstart = values_prefix_len(q);
    if (far && o.slice_walk && q.l == 1 && !long_outer) {
        // few long vectors against an inner-indexed vector far beyond L2: slices of it (and of the barcode scale, unless the mapped
        // values are materialized) staged in LDS
        r.materialized = values_wanted(q, r.fstart);
        if (slice_walk_chain(q, r.materialized ? r.fstart : 0, r.lazy_scale)) {
            r.family = SPMM_SLICE_WALK;
            return r;
        }
        r.materialized = r.lazy_scale = false;
    }
    if (far) { // the vector does not fit an XCD's L2: walked in 2 MB slices
        r.family = SPMM_SPMV2D;
        // the map's first link reads a[inner] per nonzero (the barcode scale): paired with x[inner] in one 16-byte slot
        r.fused = q.l == 1 && q.ldx == 2 && q.n_links >= 1 && q.kind[0] == OP_SCALE_AXIS && !q.a_outer[0];
        return r;
    }
    if (o.spmv_lds && q.l == 1 && !path_plain_gather(o) && q.nnz >= o.blocked_min_nnz && q.n_outer >= SPMV_LDS_MIN_OUTER && q.n_inner >= SPMV_LDS_MIN_INNER &&
        q.n_inner <= SPMV_LDS_MAX_INNER) {
        r.family = SPMM_SPMV_LDS; // vector of 64 KB .. 1.1 MB against many outer vectors: LDS-staged parts
        // a chain of the count and the outer position alone: looked up by count from a table the wave makes per row — no materialized values
        bool outer_only = o.spmv_row_table != 0 && q.n_links > 0;
        for (int i = 0; i < q.n_links && outer_only; i++) outer_only = !link_binomial(q.kind[i]) && (q.kind[i] != OP_SCALE_AXIS || q.a_outer[i]);
        r.materialized = !outer_only && values_wanted_for_alu(q, r.fstart);
        r.vm = outer_only ? 2 : r.materialized ? 1 : 0;
        return r;
    }
    r.family = SPMM_SPMV;
    return r;
}
// tiles_available: the layout exists or was built (the one impure step: spmm_tiles_auto / the forced build)
inline SpmmRoute spmm_route(const SpmmQuery &q, bool tiles_available) {
    return tiles_available && tiles_static_candidate(q) ? tile_route(q) : route_below_tiles(q);
}

} // namespace scanrs
