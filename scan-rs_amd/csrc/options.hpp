// options.hpp — every per-handle knob, as one plain value: Storage::opt holds the handle's, SpmmQuery::o a copy for the route
// decision. The comments here are the knobs' documentation beside include/scanrs_amd.h; the keys, their ranges and what stores
// them are the tables of options.cpp ("options and counters").
#pragma once
#include <cstddef>
#include <cstdint>

namespace scanrs {

struct Options {
    int spmm_path = 0;                    // 0 auto, 1 plain gather, 2 L2-blocked gather, 3 hybrid: LDS-staged tiles + gather of the overflow (tiles.hip)
    uint32_t tile_k = 2, tile_s = 32;     // hybrid product: record positions per (outer vector, visit), outer vectors per wave
    uint32_t tile_ku = 1;                 // ... unit positions among them (0 or 1; used with tile_k 2): count-1 nonzeros, added without a weight
    uint32_t tile_t = 48, tile_b = 4;     // ... panel rows per tile (<= 24 tile_k) and tile buffers in the LDS ring (tile_t * tile_b <= 192)
    int side_build = 1;                   // solvers: the second product's copy / tile layout on a helper thread beside the first pass (0: built on demand by the caller's thread)
    int tile_split = 1;                   // tile layout: slots per outer vector from its density (several for dense vectors, none — all overflow — for very sparse ones); 0: one slot per vector
    double tile_split_x = 1.8;            // ... nonzeros per panel tile a slot is sized for
    double tile_split_min = 0.5;          // ... vectors below this many nonzeros per tile get no slot
    int tile_build_one_pass = 1;          // wave-level layout builder: records and overflow in ONE walk over the matrix + a compaction (0: counting pass, then fill pass)
    int tile_weights_wide = 1;            // weight refresh of a unit-mode layout: four positions per thread with wide loads / stores (0: one position per thread)
    int tile_dense = 1;                   // tile layout of the default shape: 1 = dense record streams, accumulators picked through VGPR index mode (round 5, tiles_dense.inc); 0 = fixed positions per (slot, visit) (round 4)
    int tile_sort_slots = 2;              // dense tile layout: 2 = the slots sorted by load and DEALT over the groups (every group one slot of every load stratum: equal items, lockstep through the panel's tiles), 1 = consecutive ranks per group, 0 = vector order
    int tile_emit_staged = 1;             // dense tile layout: the stream emission keeps its tables in LDS (0: searches them in global memory, the form for parts of > 4 000 tiles)
    int tile_wtab = 1;                    // dense tile layout, folded separable map: the product kernel gathers a position's weight from the map's table by the record itself - the map evaluated inside the kernel, no weight stream (0: one f64 per position, refreshed per normalize)
    int tile_fold = 1;                    // dense tile layout, separable map: the factor of the side without the nonlinear links stays out of the per-position weights (0: both factors in every weight)
    uint64_t tile_big_list_cap = 0;       // dense tile layout, one-walk build: capacity of the list of nonzeros with counts above 255 (0: max(4 M, nnz / 64)); beyond it the two-walk build takes over
    int tile_one_walk = 1;                // dense tile layout: built in one walk over the matrix (0: count walk + fill walk; the same layout)
    int tile_builder = 1;                 // layout builder: 1 = wave-level (a lane per vector, visits in lock-step, rows written whole; default shape only), 0 = per-thread walk
    uint32_t tile_build_waves = 0;        // ... its waves per CU through a dummy LDS allocation (0: no cap — measured the same at 8, 16, 32 and without; and a builder that asks for LDS cannot run beside the persistent tile kernel of a first pass)
    size_t ov_tile_bytes = 0;             // hybrid product: panel slice per step of the overflow gather (0 = twice l2_tile_bytes)
    double tile_max_overflow = 0.35;      // auto path: an orientation whose layout would leave more than this share of the nonzeros to the overflow gather stays on the gather kernels
    int tile_auto = 1;                    // auto path may use the hybrid product (0: only spmm_path 3 does)
    int tile_overlap = 1;                 // hybrid product: 1 = the overflow gather runs beside the tile kernel (own stream); 0 = after it (measurement)
    int panel_precision = 0;              // 0: f64 panels (default); 1: gathered panels rounded to f32, f64 sums (opt-in)
    int subset_scatter = 1;               // integer sums over a column list when only the other orientation exists: 1 = scattered into the result with 64-bit integer atomics from the copy that exists, 0 = the missing copy is built (subset_host.cpp)
    uint32_t sseq_grid_cap = 16384;       // workgroups of the moment / group pass and the class walk at most (option "sseq_grid_cap": a small cap makes every wave take several outer vectors, for tests)
    int merge_fused = 1;                  // merge_clusters: 1 = one grouped pass per call, candidates from its sums; 0 = params + pairwise DE per candidate (the reference's calls)
    size_t l2_tile_bytes = 3584u << 10;   // panel slice per step of the L2-blocked gather (4 MB L2 per XCD): whole 1024-row base tiles up to 3.5 MB — 4 tiles (3.2 MB) at 100 columns, 3 (2.9 MB) at 122; measured 40.55 / 39.71 ms per pass against 41.30 / 40.23 with 3 tiles and 40.86 / 39.61 with 5, and 4 tiles of 122 columns (3.9 MB) lose 1.8 ms
    int spmm_order = 1;                   // L2-blocked gather: launch outer vectors longest first: 0 never, 1 auto, 2 always (SCANRS_SPMM_ORDER)
    uint32_t hot_segment = 512;           // ... and give a workgroup to vectors with >= this many nonzeros per step (0 = never)
    uint64_t blocked_min_nnz = 1ull << 22; // auto: matrices below this stay on the plain gather kernel
    int slice_walk = 1;                   // Ix1 products / moments on the short-outer copy stage the inner-indexed arrays in LDS slices
    int spmv_lds = 1;                     // Ix1 products on the long-outer copy stage the vector in LDS parts
    int dense_side_no_lds = 0;            // dense kernels queued on the side streams use the register-only MFMA forms (they can run BESIDE the persistent tile kernel, which holds the LDS)
    int overlap = 1;                      // small dense work of the solvers on a second stream beside the sparse passes
    int col_moments = 1;                  // per-axis sums of a log-normalized map from the copy whose OUTER vectors are summed over (per-cell table + LDS fixed-point scatter) when eligible; 0: always the ordinary pass
    int device_factor = 1;                // svd_bk: CholeskyQR factors and the coefficient bookkeeping on the device, no host round trip per orthonormalisation (0: host)
    unsigned d2h_threads = 4;             // host threads that empty the pinned ring of a large result download
    int tile_poison_slack = 0;            // test hook: launch_spmm_tiles fills the slack rows behind its compact panel copy with NaN before the tile kernel (results must not change)
    int tile_spare_cus = 1;               // the persistent tile kernel launches only as many workgroups as its number of item rounds needs; the CUs left over serve the side streams during the pass (0: a workgroup on every CU)
    int spmv_row_table = 1;               // Ix1 products over many short outer vectors: a map of the count and the outer position alone is looked up from a per-vector table instead of materialized per nonzero (0: materialized values)
    int gemm_direct = 1;                  // dense X W: operands straight from memory into the MFMA registers (0: the LDS-tiled kernels)
    double reuse_cmax = 1e5;              // svd_bk: coefficient bound above which a projection column is recomputed directly
    int materialize = 1;                  // keep the map prefix's values per nonzero on the short-outer copy (SCANRS_MATERIALIZE=0: off)
};

// options.cpp: fills `o` from the 18 values of scanrs_host_spmm_route's `options` array, each checked like the option of its name
void options_from_route_array(const double *values, Options &o);

} // namespace scanrs
