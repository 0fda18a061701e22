/*
 * scanrs_amd.h — C ABI of the MI355X (gfx950) implementation of scan-rs's
 * sparse-count-matrix normalize -> PCA hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, opaque handle,
 * create -> operate -> free, exactly the style the reference itself uses for its
 * one native component (bhtsne/src/bindings.rs:8-31).  Each entry point names
 * the reference interface it replaces (paths relative to 10XGenomics/scan-rs).
 * INTEGRATION.md shows the Rust `extern "C"` block and the `DataMat` / `Dot` /
 * `Pca` impls a maintainer would add on the reference side.
 *
 * Conventions
 *  - Matrices keep the reference orientation: `rows x cols`, `storage` 0 = CSR,
 *    1 = CSC (same u8 code as sqz/src/mat.rs:45-65). Cell Ranger's matrix is
 *    features x barcodes.
 *  - Dense panels are row-major, standard layout (sqz/src/prod.rs:102-106), f64
 *    unless the name says u32.
 *  - All functions return a status (0 = ok); they never unwind.  The message
 *    for the calling thread's last failure is scanrs_last_error().
 *  - Host pointers are borrowed for the duration of the call; the library owns
 *    the device copies inside the handle.  A handle is not thread-safe;
 *    distinct handles are independent.
 *  - There is no CPU fallback: every compute entry point needs a gfx950 device
 *    and fails with SCANRS_ERR_DEVICE otherwise.
 */
#ifndef SCANRS_AMD_H
#define SCANRS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct scanrs_mat scanrs_mat; /* opaque: AdaptiveMat / LowRankOffset on the device */

/* status codes (anyhow errors / panics / CancellationError of the reference) */
enum {
    SCANRS_OK = 0,
    SCANRS_ERR_SHAPE = 1,     /* "The input matrix must be at least 2x2." / "Dimension mismatch" */
    SCANRS_ERR_INVALID_K = 2, /* "invalid k" (bk_svd.rs:77-79) */
    SCANRS_ERR_CANCELLED = 3, /* snoop::CancellationError (snoop/src/lib.rs:5-18) */
    SCANRS_ERR_DEVICE = 4,    /* no gfx950 device / HIP failure / out of memory */
    SCANRS_ERR_NUMERICAL = 5, /* LAPACK-style failure (`?` on qr()/svddc_into()) */
    SCANRS_ERR_ARGUMENT = 6,  /* null pointer, bad enum, unsupported combination */
    SCANRS_ERR_INVALID = 6,   /* the same code under the name the select calls use: an index outside the matrix (the reference panics) */
    SCANRS_ERR_IO = 7         /* file missing / not HDF5 / truncated / a format feature this reader does not parse */
};

/* storage flag, sqz/src/mat.rs:45-65 */
enum { SCANRS_CSR = 0, SCANRS_CSC = 1 };

/* scalar maps (`ScalarMap`, sqz/src/matrix_map.rs:269-308; closures of normalization.rs:172-176, mat.rs:995) */
enum { SCANRS_FN_LN_1P = 2, SCANRS_FN_LOG2_1P = 3, SCANRS_FN_LOG10_1P = 4, SCANRS_FN_SQUARE = 5 };

/* `enum Normalization`, scan-rs/src/normalization.rs:11-28 (same order) */
enum {
    SCANRS_NORM_CELLRANGER = 0,
    SCANRS_NORM_CELLRANGER8 = 1,
    SCANRS_NORM_SEURATLOG = 2,
    SCANRS_NORM_BINOMIAL_DEVIANCE = 3,
    SCANRS_NORM_BINOMIAL_PEARSON = 4,
    SCANRS_NORM_WITH_SIZE_FACTORS = 5,
    SCANRS_NORM_LOG_TRANSFORM = 6
};

const char *scanrs_last_error(void);
/* 1 if a gfx950 device is usable from this process, else 0 (never fails). */
int scanrs_device_available(void);
const char *scanrs_version(void);

/* ---- storage: sqz::AdaptiveMat (sqz/src/mat.rs:34-42) ---------------------- */

/* AdaptiveMat::from_csmat (mat.rs:92-124) / hdf5-io read_adaptive_csr_matrix
 * (hdf5-io/src/matrix.rs:119-192): take a compressed matrix by its
 * indptr(u64)/indices(u32)/data(u32) triplet (host pointers), upload it.
 * Indices must be ascending within each outer vector; stored zeros are dropped
 * (AbsIter semantics, sqz/src/vec.rs:113). The map is MatrixIntoMap. */
int scanrs_mat_create(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices,
                      const uint32_t *values, scanrs_mat **out);
/* The reader's fallback for 10x matrix files whose indices are not sorted within a cell
 * (`new_from_unsorted_csc`, hdf5-io/src/matrix.rs:66-75): same as scanrs_mat_create, but every outer vector is first
 * sorted by index on the device. Repeated indices inside one vector are still an error. */
int scanrs_mat_create_unsorted(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices,
                               const uint32_t *values, scanrs_mat **out);
/* Same, the triplet already lives in device memory (copied, not adopted). */
int scanrs_mat_create_device(uint64_t rows, uint64_t cols, int storage, const uint64_t *d_indptr,
                             const uint32_t *d_indices, const uint32_t *d_values, scanrs_mat **out);

/* One sqz::AdaptiveVec as it lies in memory (sqz/src/vec.rs:1029-1053): the encoded buffers are handed over
 * untouched and decoded on the device (AbsIter::next, vec.rs:96-117: ascending positions, stored zeros skipped).
 *   kind      0 D3, 1 D4, 2 D8, 3 D16, 4 V, 5 S3, 6 S4, 7 S8  (declaration order of `enum AdaptiveVec`)
 *   len       logical length (the matrix's inner dimension)
 *   n_units   D*: = len; V: stored entries; S*: stored entries (= length of the inner dense value vector)
 *   data      D3/S3: Dense3.data (u64 words, 21 fields each, vec.rs:895-900); D4/S4: Dense4.data (two nibbles per
 *             byte, low nibble = even position, vec.rs:761-766); D8/S8, D16: DenseW.data (vec.rs:660-664); V: NULL
 *   fallback_*  the SimpleSparse fallback of the dense vector (indexes ascending; keyed by position for D*, by
 *             entry number for S*); for V the vector's own indexes / values (vec.rs:123-127)
 *   index_bytes, block_starts   CompressedIndexSparse fields (vec.rs:222-227), S* only:
 *             block_starts has round_up(len,256)/256 + 1 entries */
typedef struct scanrs_adaptive_vec {
    uint32_t kind;
    uint64_t len;
    uint64_t n_units;
    const void *data;
    uint64_t data_bytes;
    const uint32_t *fallback_indexes;
    const uint32_t *fallback_values;
    uint64_t n_fallback;
    const uint8_t *index_bytes;
    const uint32_t *block_starts;
    uint64_t n_block_starts;
} scanrs_adaptive_vec;

/* AdaptiveMat::new(rows, cols, storage, Vec<AdaptiveVec>) (sqz/src/mat.rs:68-90): `n_vecs` must be the outer
 * dimension (rows for CSR, cols for CSC) and every vector `len` the inner one. The compressed buffers
 * (about 4 kB per cell) are uploaded and expanded on the device; the handle is the same as scanrs_mat_create's. */
int scanrs_mat_create_adaptive(uint64_t rows, uint64_t cols, int storage, const scanrs_adaptive_vec *vecs, uint64_t n_vecs,
                               scanrs_mat **out);
/* Drop for AdaptiveMat / LowRankOffset (Rust `Drop`, cf. bhtsne/src/lib.rs:19-23). Null is a no-op. */
void scanrs_mat_free(scanrs_mat *m);

/* AdaptiveMat::view (mat.rs:242-245): new handle sharing the storage, same map/offset. */
int scanrs_mat_view(const scanrs_mat *m, scanrs_mat **out);
/* AdaptiveMat::t / LowRankOffset::t (mat.rs:262-270, low_rank_offset.rs:60-65): transposed view. */
int scanrs_mat_t(const scanrs_mat *m, scanrs_mat **out);

/* rows(), cols(), nnz(), storage (mat.rs:155-180) */
int scanrs_mat_shape(const scanrs_mat *m, uint64_t *rows, uint64_t *cols);
int scanrs_mat_nnz(const scanrs_mat *m, uint64_t *nnz);
int scanrs_mat_storage(const scanrs_mat *m, int *storage);

/* ---- lazy maps: sqz::MatrixMap (sqz/src/matrix_map.rs) ----------------------- */

/* set_map(MatrixIntoMap) (mat.rs:892-898): back to the raw counts; also drops the offset. */
int scanrs_mat_reset_map(scanrs_mat *m);
/* compose_map(ScaleAxis::new(Axis(axis), factors)) (mat.rs:901-913, matrix_map.rs:221-257).
 * axis 0: factors[r] * v (length rows); axis 1: factors[c] * v (length cols). */
int scanrs_mat_compose_scale_axis(scanrs_mat *m, int axis, const double *factors);
/* apply(f) = compose_map(ScalarMap::new(f)) (mat.rs:925-933); f is one of SCANRS_FN_*. */
int scanrs_mat_apply(scanrs_mat *m, int scalar_fn);
/* LowRankOffset::new(mat, u, v) (low_rank_offset.rs:26-33): u is rows x rank, v is rank x cols. */
int scanrs_mat_set_offset(scanrs_mat *m, uint32_t rank, const double *u, const double *v);

/* center / scale / scale_and_center (mat.rs:937-1001). `given` may be null
 * (means / std-devs are then computed on the device as the reference does). */
int scanrs_mat_center(scanrs_mat *m, int axis, const double *given_means);
int scanrs_mat_scale(scanrs_mat *m, int axis, const double *given_std);
int scanrs_mat_scale_and_center(scanrs_mat *m, int axis, const double *given_scaling);

/* ---- reductions (mat.rs:273-406) ------------------------------------------------ */

/* sum_axis::<u32> on the raw counts (normalization.rs:159,161). axis 0 -> cols entries. */
int scanrs_mat_sum_axis_u32(scanrs_mat *m, int axis, uint32_t *out);
/* sum_axis::<f64> of the mapped values (offset not included, as in the reference). */
int scanrs_mat_sum_axis_f64(scanrs_mat *m, int axis, double *out);
int scanrs_mat_mean_axis(scanrs_mat *m, int axis, double *out);
int scanrs_mat_mean_var_axis(scanrs_mat *m, int axis, double *mean, double *var);

/* var_axis (mat.rs:409-411): mean_var_axis(axis).1, the same bits. */
int scanrs_mat_var_axis(scanrs_mat *m, int axis, double *var);

/* to_dense (mat.rs:188-205, low_rank_offset.rs:55-57): rows x cols f64, small matrices / tests. */
int scanrs_mat_to_dense(scanrs_mat *m, double *out);

/* ---- select_rows / select_cols / partition_on_thresholds / to_csmat (sqz/src/mat.rs:207-241, 766-888, 1004-1071) ------------------
 * All four read the stored counts. The first three work on a handle whose map is the identity (as created, or after
 * scanrs_mat_reset_map) and that has no offset; a composed map, an offset or a sharded handle (scanrs_mat_set_shard*) returns
 * SCANRS_ERR_ARGUMENT with the reason in scanrs_last_error() (the reference clones the map verbatim and would index its per-axis
 * vectors with the new positions; that is not reproduced). A sharded handle is served by the collective entry points
 * scanrs_mat_select_rows_sharded / scanrs_mat_select_cols_sharded / scanrs_mat_partition_on_thresholds_sharded below, and a
 * scanrs_multi by scanrs_multi_select_rows / _select_cols / _partition_on_thresholds. Unchanged: the column-list statistics,
 * scanrs_sseq_de_pairs and scanrs_merge_clusters stay refused on a sharded handle (their collective forms are
 * scanrs_sseq_de_pairs_sharded and scanrs_merge_clusters_sharded), and scanrs_mat_to_adaptive exports a rank's own
 * shard only (the whole matrix of a scanrs_multi, in either orientation: scanrs_multi_to_adaptive). Transposed views work: rows of the view are columns of the stored matrix,
 * and a result's storage flag is the view's (scanrs_mat_storage). Every result is a fresh, independent handle with its own
 * storage, default options and the identity map, made on the device from the handle's own storage (no transposed copy is built, nothing
 * goes through the host); the source may be freed first. Free results with scanrs_mat_free.
 *
 * `select_rows` / `select_cols` (mat.rs:1004-1071): idx holds n_idx valid positions of that axis in any order, repeats allowed. Row i
 * of select_rows is source row idx[i]; the other dimension and the storage flag are unchanged; the inner indices of every outer
 * vector ascend. An index outside the matrix returns SCANRS_ERR_INVALID (the reference panics). n_idx = 0 gives a matrix with an
 * empty dimension, as scanrs_mat_create accepts one. */
int scanrs_mat_select_rows(scanrs_mat *m, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out);
int scanrs_mat_select_cols(scanrs_mat *m, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out);
/* `partition_on_thresholds(row_threshold, col_threshold)` (mat.rs:766-888); each threshold may be NULL (None), and
 * `partition_on_threshold(t)` is both pointing at t. A round: if a column threshold is given, the column sums over the rows not yet
 * excluded, and every column with sum < threshold joins the excluded columns; then the same for the rows over the columns not yet
 * excluded (the columns as just updated); rounds repeat until one adds nothing. Sums are exact u64 integers converted to f64 for the
 * comparison (a NaN threshold excludes nothing). One flag per round comes back to the host. Outputs, the reference's 4-tuple:
 * *filtered = kept rows x kept columns, *residual = kept rows x excluded columns (ascending source order), both with the view's
 * storage flag; either pointer may be NULL, then that matrix is not built. selected_rows / selected_cols: caller's arrays of rows /
 * cols entries, filled with the kept positions (ascending) and their counts. When everything is excluded the matrices have empty
 * dimensions. The counter "partition_rounds" (scanrs_mat_get_counter on m) holds the rounds of the last call, the final round that
 * changes nothing included. */
int scanrs_mat_partition_on_thresholds(scanrs_mat *m, const double *row_threshold, const double *col_threshold, scanrs_mat **filtered,
                                       scanrs_mat **residual, uint64_t *selected_rows, uint64_t *n_selected_rows, uint64_t *selected_cols,
                                       uint64_t *n_selected_cols);
/* The same three calls on a sharded handle (scanrs_mat_set_shard / scanrs_mat_set_shard_comm, the shards of a scanrs_multi). They are
 * COLLECTIVE: every rank calls them with the same arguments. The plain functions above stay as they are and keep refusing a sharded
 * handle. On a handle that is not sharded these give what the plain ones give. The convention is that of the sharded sSeq calls:
 * every argument and output that runs along the sharded dimension spans the WHOLE matrix, and is the same on every rank. The sharded
 * dimension is the outer dimension of the stored matrix: the rows of a handle created CSR, the columns of one created CSC, and the
 * other one of its transposed view. scanrs_mat_shape of a sharded handle keeps reporting the LOCAL count along that dimension and
 * the full extent along the other; scanrs_mat_shard_info gives the rest, and the caller sizes selected_rows / selected_cols with
 * outer_global entries along the sharded dimension and the shape's extent along the other. The preconditions of the plain functions
 * stand, with the same messages (identity map, no offset, dimensions below 2^31 - 1, taken over the global extent); transposed
 * views work as they do unsharded.
 *
 * Results: fresh independent handles (default options, identity map, own storage) made on the device from the rank's own shard,
 * already bound as rank r of the same world on the same transport as the source (the scanrs_comm, or the host hook and its ctx, which
 * must outlive them too), sharded over the same physical dimension, with their own outer_begin / outer_global. scanrs_normalize, the
 * solvers, scanrs_sseq_*, scanrs_mat_group_sums and these calls accept them, by collective calls on all ranks. A rank may end up
 * with no outer vector at all: a valid empty shard. Nothing is rebalanced.
 *
 * select: a list along the replicated (inner) dimension may be in any order, with repeats; every rank selects from its shard, the
 * ranges stay, nothing is exchanged. A list along the sharded dimension holds global positions and must not descend (repeats are
 * allowed): rank r takes the run of entries inside its range, the result's outer_begin is the number of entries below that range,
 * its outer_global is n_idx; nothing is exchanged. A list that descends returns SCANRS_ERR_ARGUMENT naming the first offending entry
 * (moving vectors between ranks is not supported); an index outside the global extent returns SCANRS_ERR_INVALID. Both are found on
 * every rank before any collective step.
 *
 * partition: the rounds of scanrs_mat_partition_on_thresholds with the sums along the replicated dimension all-reduced (u64, exact),
 * so the kept lists, both matrices (shards concatenated in rank order) and "partition_rounds" equal the unsharded call's bit for
 * bit whatever the cut. selected_rows / selected_cols are the global kept lists. *filtered and *residual follow the same rule: each
 * rank holds the part made from its own outer vectors. Every exchange is a u64 sum (the host hook sees dtype 1 only). The counter
 * "partition_allreduces" (scanrs_mat_get_counter on m) holds the exchange steps of the last call: per round one for the sums when the
 * replicated dimension has a threshold and one for the round's flag when the sharded dimension has one, plus one for the mask of the
 * sharded dimension at the end. */
int scanrs_mat_select_rows_sharded(scanrs_mat *m, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out);
int scanrs_mat_select_cols_sharded(scanrs_mat *m, const uint64_t *idx, uint64_t n_idx, scanrs_mat **out);
int scanrs_mat_partition_on_thresholds_sharded(scanrs_mat *m, const double *row_threshold, const double *col_threshold,
                                               scanrs_mat **filtered, scanrs_mat **residual, uint64_t *selected_rows,
                                               uint64_t *n_selected_rows, uint64_t *selected_cols, uint64_t *n_selected_cols);
/* Where a handle lies in a sharded matrix: its rank and world, the global position of its first outer vector and the global extent
 * of the sharded dimension. A handle that is not sharded: 0, 1, 0 and its own outer extent. Any pointer may be NULL. */
int scanrs_mat_shard_info(const scanrs_mat *m, uint32_t *rank, uint32_t *world, uint64_t *outer_begin, uint64_t *outer_global);
/* `base_mat_csc` / `to_csmat` of the stored counts (mat.rs:207-241, 257-259): indptr (outer dimension + 1 entries), indices and values
 * (scanrs_mat_nnz entries each) in the handle's own storage flag (scanrs_mat_storage: for CSR the outer dimension is the rows). The
 * map is not applied. */
int scanrs_mat_to_csmat(scanrs_mat *m, uint64_t *indptr, uint32_t *indices, uint32_t *values);

/* ---- to_adaptive: the stored counts as sqz::AdaptiveVec encodings (sqz/src/mat.rs:92-124, sqz/src/vec.rs:1086-1160) -----------------
 * The way back into the caller's own type: what scanrs_mat_create_adaptive takes, made on the device from the handle's own
 * storage (about half the bytes of the triplet of scanrs_mat_to_csmat for single-cell counts, and no AdaptiveVec::new per vector on
 * the caller's side). Bit for bit what the reference's constructors build: `choose_storage` (vec.rs:1086-1131, including the S8
 * branch that does not lower min_size), Dense3 / Dense4 / DenseW / SimpleSparse / CompressedIndexSparse::construct. Integer work
 * without atomics: two calls return the same bytes.
 *
 * Like scanrs_mat_to_csmat it reads the stored counts: a composed map or an offset is ignored, a transposed view exports the same
 * vectors under the other storage flag (scanrs_mat_storage), a sharded handle exports its own shard (the whole matrix of a
 * scanrs_multi: scanrs_multi_to_adaptive, below). The export owns two host
 * arenas (one device-to-host copy each; pinned memory from the library's pool from 1 MB on, plain heap memory below that) and the table of scanrs_adaptive_vec whose pointers lead into them, each aligned for
 * its element type; the device arenas are released before the call returns. */
typedef struct scanrs_adaptive_export scanrs_adaptive_export;
/* AdaptiveMat::from_csmat / AdaptiveVec::new per outer vector (mat.rs:92-124, vec.rs:1086-1160), run on the device.
 * force_kind: -1 = choose_storage, 0..7 = that encoding for every vector (the `kind` codes of scanrs_adaptive_vec); anything else is
 * SCANRS_ERR_ARGUMENT. A matrix without outer vectors and empty vectors are valid. Free the result with
 * scanrs_adaptive_export_free. */
int scanrs_mat_to_adaptive(scanrs_mat *m, int force_kind, scanrs_adaptive_export **out);
/* The same with the orientation of the table chosen. SCANRS_EXPORT_STORED is scanrs_mat_to_adaptive: one vector per stored outer
 * vector. SCANRS_EXPORT_INNER encodes the handle's OTHER copy (the transposed orientation, built on first use as the products build
 * it and kept by the handle): n_inner vectors of len = n_outer, the table scanrs_mat_create_adaptive(rows, cols, the OTHER storage
 * flag, ...) takes - for a genes x cells matrix stored cell-major, one vector per gene, the reference's own orientation
 * (hdf5-io/src/matrix.rs:119-192). Through a transposed view the majors swap nothing else: the vectors are those of the stored
 * arrays, the flag is the view's. Map and offset are ignored, as above. STORED on a sharded handle exports the rank's own shard;
 * INNER on a sharded handle is SCANRS_ERR_ARGUMENT (no rank holds a whole inner vector: scanrs_multi_to_adaptive). major outside
 * 0..1, force_kind outside -1..7 and a null argument are SCANRS_ERR_ARGUMENT, before any device work. */
enum { SCANRS_EXPORT_STORED = 0, SCANRS_EXPORT_INNER = 1 };
int scanrs_mat_to_adaptive_major(scanrs_mat *m, int major, int force_kind, scanrs_adaptive_export **out);
/* n_vecs: the entries of the table (the outer dimension; the inner one for SCANRS_EXPORT_INNER). total_bytes: the sum of the reference's mem_size() — data + 8 per fallback entry (+ index bytes + 4
 * per block start for S*; 8 per entry for V). kind_counts[k]: vectors of encoding k. Each output pointer may be NULL. */
int scanrs_adaptive_export_info(const scanrs_adaptive_export *e, uint64_t *n_vecs, uint64_t *total_bytes, uint64_t kind_counts[8]);
/* The table (n_vecs entries), borrowed until scanrs_adaptive_export_free; it can be passed straight to
 * scanrs_mat_create_adaptive(rows, cols, storage, vecs, n_vecs, ...). */
int scanrs_adaptive_export_vecs(const scanrs_adaptive_export *e, const scanrs_adaptive_vec **vecs);
void scanrs_adaptive_export_free(scanrs_adaptive_export *e); /* NULL is a no-op */
/* Host side of the header both compile: the kind AdaptiveVec::new would pick for a vector of length `len` with these n stored
 * values, and the reference's second result, the smallest size estimate seen before the S8 and V branches (min_size may be NULL).
 * Needs no device. */
int scanrs_host_choose_storage(uint64_t len, const uint32_t *values, uint64_t n, int *kind, uint64_t *min_size);

/* ---- products: `Dot` impls (mat.rs:1074-1170, low_rank_offset.rs:68-96, prod.rs) -- */

/* self.dot(rhs): rhs is cols x l, out is rows x l (includes the offset u*(v*rhs) when set). */
int scanrs_mat_dot(scanrs_mat *m, const double *rhs, uint32_t l, double *out);
/* lhs.dot(self): lhs is l x rows, out is l x cols. */
int scanrs_mat_rdot(scanrs_mat *m, const double *lhs, uint32_t l, double *out);
/* The `A = u32` instantiation tested by mat.rs:1406-1486 / benched by
 * sqz/benches/my_benchmark.rs (identity map, wrapping integer arithmetic). */
int scanrs_mat_dot_u32(scanrs_mat *m, const uint32_t *rhs, uint32_t l, uint32_t *out);
int scanrs_mat_rdot_u32(scanrs_mat *m, const uint32_t *lhs, uint32_t l, uint32_t *out);
/* Device-resident panels, padded leading dimensions (elements): d_out[rows x l] = self * d_rhs[cols x l];
 * with `transpose` != 0: d_out[cols x l] = self^T * d_rhs[rows x l]. ld must be even. */
int scanrs_mat_dot_device(scanrs_mat *m, int transpose, const double *d_rhs, uint32_t ld_rhs, uint32_t l, double *d_out,
                          uint32_t ld_out);

/* ---- normalization: scan-rs/src/normalization.rs ----------------------------------- */

/* normalize / normalize_with_size_factor (normalization.rs:46-102) and the binomial
 * residual maps (:232-322): installs the lazy map + rank-1 offset on the handle.
 * size_factors (length cols) only for SCANRS_NORM_WITH_SIZE_FACTORS, else null. */
int scanrs_normalize(scanrs_mat *m, int normalization, const uint32_t *size_factors);
/* log_normalize_with_size_factor (normalization.rs:138-178) without the centre/scale step.
 * umi_count_sum < 0 means None (median of the column sums). */
int scanrs_log_normalize(scanrs_mat *m, double umi_count_sum, int log_fn, const uint32_t *size_factors);
/* log1p_normalize_fixed_point (normalization.rs:191-213). */
int scanrs_log1p_normalize_fixed_point(scanrs_mat *m, int log_fn, uint32_t base, uint32_t exponent);
/* target UMI count chosen by the last (log_)normalize call: max(median(colsums), 1) (normalization.rs:162-168) */
int scanrs_mat_target_umi(const scanrs_mat *m, double *target);

/* ---- PCA: scan-rs/src/dim_red ----------------------------------------------------------- */

/* snoop::CancelProgress (snoop/src/lib.rs:37-58): `cancel` points at an
 * AtomicBool-compatible byte read with relaxed ordering between kernel launches
 * (may be null); `progress` receives set_progress fractions (may be null). */
typedef void (*scanrs_progress_fn)(void *ctx, double fraction);
typedef struct {
    const volatile uint8_t *cancel;
    scanrs_progress_fn progress;
    void *ctx;
} scanrs_snoop;

/* ---- statistics over a list of columns: sum_rows / sum_cols / sum_rows_dual / mean_rows / mean_var_rows -------------------------------
 * sqz/src/mat.rs: sum_rows::<O>(cols) :449-481, sum_cols::<O>(cols) :414-446, sum_rows_dual[_with_cancellation]::<O>(cols1, cols2)
 * :484-583, mean_rows(cols) :279-282, mean_var_rows(cols) :333-374 — what the reference's own DE is written in (diff_exp.rs:143 calls
 * sum_rows_dual_with_cancellation::<u64>, :317 sum_cols::<f64>, :469 and :524 mean_var_rows, :574-575 sum_rows::<u64>).
 * Rows and columns are the view's (scanrs_mat_t swaps them); every call works on a CSR handle, a CSC handle and a transposed view.
 *
 * A list holds n indices of view columns, STRICTLY ASCENDING and in range ("must be sorted", mat.rs:413 / :448; a repeated index is
 * refused as scanrs_sseq_params refuses it): anything else returns SCANRS_ERR_ARGUMENT, with the list's name in scanrs_last_error(),
 * before any device work. An empty list (n = 0, the pointer may be NULL) is valid: sums are 0, means and variances NaN (0.0 / 0.0, as
 * in the reference). cols1 and cols2 of the dual forms may overlap; a column in both counts in both results.
 *   sum_rows      out[r] (rows entries) = the sum of row r over the listed columns
 *   sum_cols      out[i] (n entries)    = the sum of column cols[i] over all rows
 *   sum_rows_dual out1 / out2 (rows entries each) = sum_rows over cols1 / cols2, from one walk over the matrix
 *   mean_rows     sum_rows_f64 / n;  mean_var_rows: mean and E[x^2] - E[x]^2 of the mapped values over the listed columns
 * The _u64 results are defined on the raw counts: a handle whose map is not the identity is refused (as scanrs_mat_sum_axis_u32);
 * they are exact (three counts of 4294967295 in a row give 12884901885). The f64 results apply the handle's map per nonzero (stored
 * zeros and absent entries contribute nothing; a low-rank offset is left out, as scanrs_mat_mean_var_axis leaves it out). They use no
 * floating-point atomics and are bit-reproducible: two calls give identical arrays, also after other calls on the handle and on a
 * fresh handle. A sharded handle returns SCANRS_ERR_ARGUMENT from these plain calls; the collective *_sharded forms below serve it.
 * The kernel form follows the copy that exists: a masked walk when the result axis is the copy's outer
 * dimension, a walk over the listed vectors when the listed columns are outer vectors; integer results whose copy does not exist are
 * scattered from the other copy with 64-bit integer atomics instead of building it (handle option "subset_scatter"), f64 results
 * build it on demand as scanrs_mat_mean_var_axis does. Counters "subset_masked_passes" / "subset_scatter_passes".
 * `snoop` of the dual forms may be NULL. A cancel flag that is already set returns SCANRS_ERR_CANCELLED before anything is queued;
 * otherwise the flag is read between launches; a cancelled call leaves out1 / out2 untouched. Progress is nondecreasing, starts at
 * 0.0 and ends at 1.0 (mat.rs:519, :581).
 * NOT provided: sum_cols_diff (mat.rs:612-722). Nothing in the reference calls it, its norm_factors branches are recurrences that
 * read like defects ((acc + v m) / f folded along the vector; an integer division by a truncated factor), and its CSC branch
 * accumulates in u32. (Declared here, behind scanrs_snoop, which the dual forms take.) */
int scanrs_mat_sum_rows_u64(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out);
int scanrs_mat_sum_rows_f64(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out);
int scanrs_mat_sum_cols_u64(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out);
int scanrs_mat_sum_cols_f64(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out);
int scanrs_mat_sum_rows_dual_u64(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                 const scanrs_snoop *snoop, uint64_t *out1, uint64_t *out2);
int scanrs_mat_sum_rows_dual_f64(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                 const scanrs_snoop *snoop, double *out1, double *out2);
int scanrs_mat_mean_rows(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out);
int scanrs_mat_mean_var_rows(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *mean, double *var);

/* The same eight calls on a sharded handle (scanrs_mat_set_shard / scanrs_mat_set_shard_comm, the shards of a scanrs_multi; DESIGN.md
 * section 7k). They are COLLECTIVE: every rank calls them with the same arguments. On a handle that is not sharded they are the plain
 * calls: the same kernels, the same bits. The convention is that of the sharded sSeq and select calls: the sharded dimension is the
 * outer dimension of the stored matrix (the other one of a transposed view); a list along it holds GLOBAL indices and is checked
 * against the global extent, with the plain calls' rules and messages; an output along it spans the WHOLE matrix (outer_global
 * entries); every output is complete and identical on every rank. An offset is left out, as above. Only u64 sum all-reduces cross
 * the shards (dtype 1 of scanrs_allreduce_fn), so no result depends on the cut into shards, the number of ranks or the transport:
 *   - A result that runs ALONG the sharded dimension (sum_rows, sum_rows_dual, mean_rows, mean_var_rows when the view's rows are
 *     sharded; sum_cols when its columns are) is owned by one rank, which computes it with the plain kernels on its own storage from
 *     its part of the list; one all-reduce over the bit patterns of a zero-filled array of the whole extent copies it to everyone.
 *     Under a map that holds the same numbers these results equal the unsharded call's bit for bit.
 *   - A sum that CROSSES the shards (the sum_rows family when the view's columns are sharded - genes x cells with lists of cells, the
 *     scanrs_multi shape; sum_cols when its rows are). u64: the partial sums are added by one all-reduce, exact, the unsharded call's
 *     bits. f64: fixed point. Every mapped value x is rounded ONCE to a quantum q = 1 / scale that all ranks share, and the sum of
 *     squares takes the f64 product x * x, rounded once to a quantum of its own; the rounded terms are added as signed 128-bit
 *     integers (two's complement, so terms of either sign are served) and cross the shards as 32-bit limbs; the host converts the
 *     integer sum to f64 (one rounding) and divides by the scale (exact). No floating-point addition lies between a term and that
 *     conversion. THE QUANTUM: scale = 2^(123 - ilogb(bound)), bound = M x T, where M is the largest finite |x| over the listed
 *     nonzeros of ALL shards (found by a pre-pass; rank r's value travels as a bit pattern in slot r of a zeroed world-long u64
 *     array, the host takes the maximum) and T the largest number of terms a result can have: the length of the list for the
 *     sum_rows family (the longer list of a dual call; both sums share the quantum), the global number of rows for sum_cols. The sum
 *     of squares uses bound = (M x M) x T. Every sum then stays below 2^124 and the result is within T / 2 quanta - below 2^-90 of
 *     the bound - of the exact sum of the f64 terms. A bound of 0 (nothing listed) gives scale 1; bounds below 2^-877 give 2^1000.
 *     A result that met a term that is not finite is returned as NaN, in that result alone: the one place where a value can differ
 *     in KIND from the unsharded call, which would propagate an infinity. (So is a sum of squares whose bound overflows f64.)
 * mean_rows and mean_var_rows divide on the host as the plain calls do. `snoop` of the dual forms: every rank polls its snoop at
 * the same checkpoints and must see the same flag; a cancelled call leaves out1 / out2 untouched on every rank.
 * Counter "subset_allreduces" = the exchange steps of the last of these calls on the handle: 0 on an unsharded handle and for
 * outputs without entries, 1 for results along the sharded dimension and for u64 sums that cross the shards, 2 for f64 sums that
 * cross them (the pre-pass's maximum, then the limbs: 5 u64 per 128-bit sum and result). */
int scanrs_mat_sum_rows_u64_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out);
int scanrs_mat_sum_rows_f64_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out);
int scanrs_mat_sum_cols_u64_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, uint64_t *out);
int scanrs_mat_sum_cols_f64_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out);
int scanrs_mat_sum_rows_dual_u64_sharded(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                         const scanrs_snoop *snoop, uint64_t *out1, uint64_t *out2);
int scanrs_mat_sum_rows_dual_f64_sharded(scanrs_mat *m, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                         const scanrs_snoop *snoop, double *out1, double *out2);
int scanrs_mat_mean_rows_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *out);
int scanrs_mat_mean_var_rows_sharded(scanrs_mat *m, const uint64_t *cols, uint64_t n, double *mean, double *var);

/* BkSvd::run_pca_cancellable / svd_bk (dim_red/bk_svd.rs:41-146).
 * omega: optional explicit start panel in the reference's own layout
 * ((cols x b) row-major when rows >= cols, else (b x rows)), b = min(rows, cols, ceil(k*k_multiplier));
 * null -> generated from `seed` like SmallRng::seed_from_u64 + Uniform(-1,1).
 * Outputs (caller-allocated, row-major): u rows x k, s k, v cols x k  (= PcaResult, dim_red/mod.rs:47).
 * u and/or v may be null: the factor then stays in device memory only (no PCIe copy). */
int scanrs_pca_bk(scanrs_mat *m, uint32_t k, double k_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
                  const scanrs_snoop *snoop, double *u, double *s, double *v);
/* RandSvd::run_pca / svd_rand (dim_red/rand_svd.rs:37-129). l = max(k+4, (k*l_multiplier) as usize).
 * omega layout: (cols x l) when rows >= cols, else (l x rows). */
int scanrs_pca_rand(scanrs_mat *m, uint32_t k, double l_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
                    double *u, double *s, double *v);
/* Irlba::run_pca_cancellable / irlba (dim_red/irlba.rs:59-215). v0: optional start vector (length cols);
 * null -> seeded normal. mprod (may be null) receives the "number of matrix products" (irlba.rs:212). */
int scanrs_pca_irlba(scanrs_mat *m, uint32_t nu, double tol, uint32_t max_iter, const double *v0,
                     const scanrs_snoop *snoop, double *u, double *s, double *v, uint32_t *mprod);
/* PcaResult of the last scanrs_pca_bk / scanrs_pca_rand call on this handle as it lies in device memory
 * (dim_red/mod.rs:47 returns owned arrays; a device consumer — scanrs_knn_device below, a clustering kernel of the
 * caller — takes them from here without the PCIe round trip): *d_u is rows x k with leading dimension *ld_u
 * (elements, row-major), *d_v is cols x k (the local columns of a sharded handle). The memory belongs to the handle
 * and is valid until its next PCA call or scanrs_mat_free. Any output pointer may be null. */
int scanrs_pca_result_device(scanrs_mat *m, const double **d_u, uint32_t *ld_u, const double **d_v, uint32_t *ld_v,
                             uint32_t *k);
/* The panel the two randomized drivers draw for a given seed (count values, row-major fill order). */
int scanrs_omega_fill(uint64_t seed, uint64_t count, double *out);

/* ---- nearest neighbours of the PCA scores: scan_rs::nn (scan-rs/src/nn.rs) -------------- */

/* knn(v, k) (nn.rs:38-57): for every row of the n x d row-major matrix `points` the indices of its k nearest OTHER rows
 * by Euclidean distance, nearest first; rows of `out` (n x k) are padded with UINT32_MAX when fewer than k exist
 * (`T::max_value()`, nn.rs:66). Exact (exhaustive search in f64 on the device); exactly equidistant neighbours come in
 * ascending index order. k <= 128, d <= 128. */
int scanrs_knn(const double *points, uint64_t n, uint32_t d, uint32_t k, uint32_t *out);
/* find_nn(v, k, tree, include_self) (nn.rs:63-83): the k nearest of `points` (the tree's point set, n_p x d) to each
 * row of `queries` (n_q x d). As in the reference, include_self = 0 drops the point whose INDEX equals the query's
 * row number, which is only meaningful when the two sets are the same. */
int scanrs_find_nn(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k,
                   int include_self, uint32_t *out);

/* scanrs_knn on points already in device memory (n x d, row-major, leading dimension ld >= d elements), e.g. the
 * scores scanrs_pca_result_device hands out; `out` (n x k) is a host array. */
int scanrs_knn_device(const double *d_points, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, uint32_t *out);

/* ---- multi-GPU: one process per GPU, cells range-partitioned ----------- */

/* In-place sum all-reduce of `count` elements of device memory across ranks.
 * dtype 0 = f64, 1 = u64. Returns 0 on success. The host program supplies it
 * (bench.py: torch.distributed over RCCL); the library calls it once per
 * sparse product that contracts over the sharded dimension. */
typedef int (*scanrs_allreduce_fn)(void *ctx, void *d_buf, uint64_t count, int dtype);
/* Declare that this handle holds outer vectors [outer_begin, outer_begin + n_local) of a
 * matrix whose sharded (outer) dimension has `outer_global` entries. The handle's own
 * shape keeps the local count; reductions over the outer dimension become global. */
int scanrs_mat_set_shard(scanrs_mat *m, uint32_t rank, uint32_t world, uint64_t outer_begin, uint64_t outer_global,
                         scanrs_allreduce_fn allreduce, void *ctx);
/* The library's own transport for the exchange steps (replaces the host hook above): RCCL over xGMI, loaded when the
 * first communicator is made. One process per GPU: rank 0 draws the 128-byte id (scanrs_comm_get_unique_id), the
 * host program passes it to the other ranks by any channel it has, every rank calls scanrs_comm_create with its
 * device current, then scanrs_mat_set_shard_comm on its handle. The collectives are enqueued on the handle's own
 * stream (no host synchronisation). The communicator is borrowed by the handle and must outlive it. */
typedef struct scanrs_comm scanrs_comm;
#define SCANRS_COMM_ID_BYTES 128
int scanrs_comm_get_unique_id(uint8_t *id /* SCANRS_COMM_ID_BYTES */);
int scanrs_comm_create(const uint8_t *id, uint32_t rank, uint32_t world, scanrs_comm **out);
void scanrs_comm_free(scanrs_comm *c);
/* The group as the transport counts it - ranks and this rank from ncclCommCount / ncclCommUserRank (the single-process form: its own
 * group) - and the sum all-reduces that went through this communicator so far (calls, payload bytes). Any pointer may be NULL. */
int scanrs_comm_info(scanrs_comm *c, uint32_t *nranks, uint32_t *rank, uint64_t *n_allreduce, uint64_t *allreduce_bytes);
int scanrs_mat_set_shard_comm(scanrs_mat *m, scanrs_comm *comm, uint32_t rank, uint32_t world, uint64_t outer_begin,
                              uint64_t outer_global);

/* Single-process form (SURVEY.md §8b `mat_create(..., n_gpus)`; Cell Ranger is one process, tools/src/bin/cmd.rs:61-70):
 * the whole matrix is handed over once, its outer vectors are range-partitioned by nonzeros over `n_shards` devices
 * (`devices` null = 0 .. n_shards-1; ids may repeat, several shards then share a device), every shard is driven by a
 * host thread of the library during a call, and the exchange steps are a one-shot reduce-scatter + all-gather over
 * peer-mapped memory. Outputs as in scanrs_pca_bk: u rows x k, s k, v cols x k for the WHOLE matrix. */
typedef struct scanrs_multi scanrs_multi;
int scanrs_multi_create(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices,
                        const uint32_t *values, uint32_t n_shards, const int *devices, scanrs_multi **out);
void scanrs_multi_free(scanrs_multi *mm);
int scanrs_multi_n_shards(const scanrs_multi *mm, uint32_t *n);
/* shard i: its handle (owned by mm; use it from a thread whose current device is *device), its range of outer vectors */
int scanrs_multi_shard(scanrs_multi *mm, uint32_t i, scanrs_mat **shard, int *device, uint64_t *outer_begin, uint64_t *outer_end);
/* scanrs_comm_info of shard i's communicator: the exchange steps of this shard so far (calls, payload bytes) */
int scanrs_multi_comm_info(scanrs_multi *mm, uint32_t i, uint32_t *nranks, uint32_t *rank, uint64_t *n_allreduce, uint64_t *allreduce_bytes);
int scanrs_multi_normalize(scanrs_multi *mm, int normalization, const uint32_t *size_factors);
int scanrs_multi_pca_bk(scanrs_multi *mm, uint32_t k, double k_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
                        const scanrs_snoop *snoop, double *u, double *s, double *v);
int scanrs_multi_pca_rand(scanrs_multi *mm, uint32_t k, double l_multiplier, uint32_t n_iter, uint64_t seed, const double *omega,
                          double *u, double *s, double *v);
int scanrs_multi_log_normalize(scanrs_multi *mm, double umi_count_sum, int log_fn, const uint32_t *size_factors);
/* v0 (optional) spans ALL columns of the matrix. */
int scanrs_multi_pca_irlba(scanrs_multi *mm, uint32_t nu, double tol, uint32_t max_iter, const double *v0, const scanrs_snoop *snoop,
                           double *u, double *s, double *v, uint32_t *mprod);
/* sSeq differential expression over the shards (see "Sharded handles" in the sSeq section below): scanrs_sseq_params,
 * scanrs_mat_group_sums and scanrs_sseq_de_backend (modes 0, 1 and 2, both backends) with the handle replaced by `mm, transposed`.
 * The cells must be the sharded dimension: a genes x cells matrix created CSC with transposed = 0, or a cells x genes matrix created
 * CSR with transposed = 1 (every shard then runs through scanrs_mat_t); anything else returns SCANRS_ERR_ARGUMENT. All per-cell
 * arguments span the whole matrix; the outputs are those of the unsharded call, bit for bit (shard 0 writes them, the other shards
 * write the same values into scratch of the call). Every shard polls the cancel flag of `snoop`, only shard 0 reports progress. */
int scanrs_multi_sseq_params(scanrs_multi *mm, int transposed, double zeta_quintile, const uint64_t *cell_indices, uint64_t n_sel,
                             const double *umi_counts, double *size_factors, double *gene_means, double *gene_variances,
                             uint8_t *use_genes, double *gene_moment_phi, double *zeta_hat, double *delta, double *gene_phi);
int scanrs_multi_group_sums(scanrs_multi *mm, int transposed, const int16_t *labels, uint32_t n_groups, uint64_t *sums,
                            uint64_t *cells_per_group);
int scanrs_multi_sseq_de(scanrs_multi *mm, int transposed, const int16_t *labels, uint32_t n_groups, int mode, const double *size_factors,
                         const double *gene_means, const double *gene_phi, const uint8_t *use_genes, uint64_t big_count, int backend,
                         const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc,
                         double *mean_in, double *mean_out);
/* The statistics over a list of columns over the shards: scanrs_mat_sum_rows_u64_sharded ... scanrs_mat_mean_var_rows_sharded (see
 * the column-list section) on every shard at once, with the handle replaced by `mm, transposed` (transposed != 0: every shard runs
 * through scanrs_mat_t; rows and columns are then those of the transposed matrix). Either dimension may be the sharded one. Lists
 * and outputs span the whole matrix; shard 0 writes the caller's arrays, the other shards write the same values into scratch of the
 * call. Every shard polls the cancel flag of `snoop`, only shard 0 reports progress. */
int scanrs_multi_sum_rows_u64(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, uint64_t *out);
int scanrs_multi_sum_rows_f64(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, double *out);
int scanrs_multi_sum_cols_u64(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, uint64_t *out);
int scanrs_multi_sum_cols_f64(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, double *out);
int scanrs_multi_sum_rows_dual_u64(scanrs_multi *mm, int transposed, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                   const scanrs_snoop *snoop, uint64_t *out1, uint64_t *out2);
int scanrs_multi_sum_rows_dual_f64(scanrs_multi *mm, int transposed, const uint64_t *cols1, uint64_t n1, const uint64_t *cols2, uint64_t n2,
                                   const scanrs_snoop *snoop, double *out1, double *out2);
int scanrs_multi_mean_rows(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, double *out);
int scanrs_multi_mean_var_rows(scanrs_multi *mm, int transposed, const uint64_t *cols, uint64_t n, double *mean, double *var);
/* The shape of the WHOLE matrix, its nonzeros over all shards and its storage flag. Any pointer may be NULL. */
int scanrs_multi_shape(const scanrs_multi *mm, uint64_t *rows, uint64_t *cols, uint64_t *nnz, int *storage);
/* scanrs_mat_to_csmat of the whole matrix, the shards concatenated: indptr (outer dimension + 1), indices and values (nnz each). */
int scanrs_multi_to_csmat(scanrs_multi *mm, uint64_t *indptr, uint32_t *indices, uint32_t *values);
/* select_rows / select_cols / partition_on_thresholds over the shards: scanrs_mat_select_rows_sharded, _select_cols_sharded and
 * _partition_on_thresholds_sharded (see the select section) on every shard at once, with the arguments and lists of the whole
 * matrix (selected_rows / selected_cols: rows / cols entries). A list along the sharded dimension (the rows of a CSR matrix, the
 * columns of a CSC one) must not descend. Every result is a new scanrs_multi on the same devices with the same number of shards,
 * with a group and communicators of its own: the source and its results may be freed in either order (scanrs_multi_free). The
 * shards are NOT rebalanced after a filter: each holds what is left of its own outer vectors, possibly none. On any failure nothing
 * is leaked and *out / *filtered / *residual are NULL. filtered / residual may be NULL (that matrix is not built). */
int scanrs_multi_select_rows(scanrs_multi *mm, const uint64_t *idx, uint64_t n_idx, scanrs_multi **out);
int scanrs_multi_select_cols(scanrs_multi *mm, const uint64_t *idx, uint64_t n_idx, scanrs_multi **out);
int scanrs_multi_partition_on_thresholds(scanrs_multi *mm, const double *row_threshold, const double *col_threshold,
                                         scanrs_multi **filtered, scanrs_multi **residual, uint64_t *selected_rows,
                                         uint64_t *n_selected_rows, uint64_t *selected_cols, uint64_t *n_selected_cols);
/* nnz-balanced contiguous partition of the outer dimension: bounds has world+1 entries. */
int scanrs_plan_shards(const uint64_t *indptr, uint64_t n_outer, uint32_t world, uint64_t *bounds);

/* ---- cell-sharded scanrs_multi from feature-major input --------------------
 * scanrs_multi_create cuts the OUTER dimension of its triplet, and everything after it (normalize, the DE calls, kNN) needs the
 * cells to be the sharded dimension - while the matrix the reference holds is feature-major: genes x cells CSR, one AdaptiveVec per
 * gene (load_mtx, scan-rs/src/mtx.rs:10-51; read_adaptive_csr_matrix, hdf5-io/src/matrix.rs:119-192; tools/src/bin/cmd.rs:61-70).
 * These constructors take the matrix in that orientation and shard its INNER dimension: the result is a scanrs_multi of the same
 * rows x cols whose storage flag is the OTHER one (a genes x cells CSR triplet gives a genes x cells CSC multi with the cells
 * sharded, a cells x genes CSC triplet a cells x genes CSR one). It equals scanrs_multi_create of the host-transposed triplet in
 * every respect: the same shard ranges (scanrs_plan_shards over the stored entries per inner position, stored zeros counted), the
 * same arrays in every shard bit for bit (indices ascending, stored zeros dropped), communicators of its own; every scanrs_multi_*
 * call works on it unchanged. Nothing is transposed on the host and every nonzero crosses the host link once: the outer vectors are
 * dealt in n_shards contiguous slabs by nonzeros (scanrs_plan_shards on the given indptr), shard s uploads slab s only -
 * 8 z + 8 (n + 1) bytes for n vectors with z entries - and the shards exchange their pieces on the devices.
 * Validation is scanrs_mat_create's (same codes and messages: an index out of range or not strictly ascending, indptr[0] != 0, null
 * arrays, dimensions beyond u32) and runs on every slab before anything is indexed by an inner index; n_shards, devices and peer
 * access are checked as in scanrs_multi_create (`devices` may repeat an id). On any failure nothing is leaked and *out is NULL.
 * Not served: the one-process-per-GPU forms (RCCL, host hook: their only transport is a sum all-reduce). (An existing scanrs_multi is
 * cut anew by scanrs_multi_rebalance, below; the way back out in this orientation is scanrs_multi_to_adaptive with
 * SCANRS_EXPORT_INNER, further down.) */
/* AdaptiveMat::new from a triplet (sqz/src/mat.rs:68-124), sharded over the inner dimension */
int scanrs_multi_create_inner(uint64_t rows, uint64_t cols, int storage, const uint64_t *indptr, const uint32_t *indices,
                              const uint32_t *values, uint32_t n_shards, const int *devices, scanrs_multi **out);
/* The same from the table scanrs_mat_create_adaptive takes (AdaptiveMat::new(rows, cols, storage, Vec<AdaptiveVec>), mat.rs:68-90;
 * what read_adaptive_csr_matrix returns, hdf5-io/src/matrix.rs:119-192). n_vecs is the outer dimension. The slabs are cut by the
 * entries the vectors store (n_units); the compressed buffers of a slab are what is uploaded, and the slab is expanded on its device.
 * The result holds the nonzeros (the decoder skips stored zeros, vec.rs:96-117). */
int scanrs_multi_create_adaptive_inner(uint64_t rows, uint64_t cols, int storage, const scanrs_adaptive_vec *vecs, uint64_t n_vecs,
                                       uint32_t n_shards, const int *devices, scanrs_multi **out);
/* (scanrs_multi_create_from_file: with the readers, below) */
/* What the constructor did: slab_bounds (n_shards + 1: the outer vectors of every slab), moved (n_shards x n_shards:
 * moved[s * n + d] = the stored entries of slab s whose inner index lies in shard d's range, stored zeros included) and
 * uploaded_bytes (one entry per shard; the AdaptiveVec form reports its compressed bytes). Any pointer may be NULL.
 * SCANRS_ERR_ARGUMENT on a scanrs_multi that no inner-sharding constructor made. */
int scanrs_multi_create_info(const scanrs_multi *mm, uint64_t *slab_bounds, uint64_t *moved, uint64_t *uploaded_bytes);
/* The same plan from host arrays, no device: slab_bounds and bounds (world + 1 entries each: the slabs of the outer dimension, the
 * shards of the inner one) and moved (world x world), validated as above. Any output may be NULL. */
int scanrs_host_plan_inner(const uint64_t *indptr, const uint32_t *indices, uint64_t n_outer, uint64_t n_inner, uint32_t world,
                           uint64_t *slab_bounds, uint64_t *bounds, uint64_t *moved);

/* ---- rebalance and any-order outer selection of a scanrs_multi -----------
 * One primitive moves outer vectors between shards: "the outer vectors idx[0 .. n_idx) of the WHOLE matrix, in that order, as a freshly
 * balanced scanrs_multi". It lifts the two restrictions of the scanrs_multi_select_* block above, which stay as they are for those
 * calls: scanrs_multi_gather_outer takes a list along the sharded dimension in ANY order (descending, shuffled, with repeats), and
 * scanrs_multi_rebalance - the identity list - cuts the unbalanced result of a filter anew by nonzeros. Another n_shards or other
 * `devices` re-shard the matrix. The result equals scanrs_multi_create(rows', cols', storage, T, n_shards, devices) for the selected
 * triplet T (outer vector j of T = vector idx[j] of the source; inner dimension and storage flag unchanged) in every respect: the same
 * bounds (scanrs_plan_shards over T's indptr), every shard's indptr, indices and values bit for bit, the largest count and the work
 * items scanrs_mat_create leaves on a handle, a group and communicators of its own (source and result may be freed in either order).
 * The source is not modified. No nonzero crosses the host link: the sources' indptr arrays go down, the destinations' slices of the
 * list go up (host_bytes, below), and every destination copies its vectors out of the sources' device arrays in place, through the
 * peer mapping where the devices differ (peer access is enabled from every destination device to every source device).
 * Preconditions, those of scanrs_multi_select_rows: identity map, no offset (scanrs_mat_reset_map), dimensions below 2^31 - 1.
 * Refusals, all before any device work: an index beyond the outer extent SCANRS_ERR_INVALID; a null list with n_idx > 0, n_shards
 * outside 1 .. 16 or a device that does not exist SCANRS_ERR_ARGUMENT; each message names the argument. On any failure nothing is
 * leaked and *out is NULL. n_idx == 0 gives what scanrs_multi_create gives for a matrix without outer vectors: a valid scanrs_multi
 * of empty shards.
 * Still out of scope: the one-process-per-GPU forms (RCCL, host hook), whose only transport is a sum all-reduce. (to_adaptive of a
 * whole scanrs_multi, which this list used to name, is served: scanrs_multi_to_adaptive, further down.) */
/* the outer vectors idx[0..n_idx) of the WHOLE matrix (global positions along the sharded = stored outer dimension; any order,
 * repeats allowed), in list order, as a new scanrs_multi over n_shards shards on `devices` (null: 0..n_shards-1; ids may repeat) */
int scanrs_multi_gather_outer(scanrs_multi *mm, const uint64_t *idx, uint64_t n_idx, uint32_t n_shards, const int *devices,
                              scanrs_multi **out);
/* the identity list: the same matrix, cut anew by nonzeros. n_shards = 0: as many shards as mm has, on mm's devices. */
int scanrs_multi_rebalance(scanrs_multi *mm, uint32_t n_shards, const int *devices, scanrs_multi **out);
/* nonzeros per shard (n_shards entries) and max/mean of them (1 for a matrix without nonzeros); works on every scanrs_multi.
 * Either output may be NULL. */
int scanrs_multi_balance(const scanrs_multi *mm, uint64_t *shard_nnz, double *imbalance);
/* what the call that made `mm` did: the source's shard count, bounds (n_shards + 1), moved (n_src x n_shards nonzeros, source-major:
 * moved[s * n_shards + d] came from source shard s to shard d) and host_bytes (n_shards entries: the bytes that crossed the host link
 * in either direction - 4 per vector of the shard's slice of the list up, 8 for the one total that comes back, and the download of
 * source shard s's indptr, 8 (n_s + 1) bytes, charged to entry s mod n_shards). Any pointer may be NULL. SCANRS_ERR_ARGUMENT on a
 * scanrs_multi these calls did not make. Per shard, scanrs_mat_get_counter "regather_plan_us" / "regather_pull_us" /
 * "regather_finish_us": wall clock of the phases. */
int scanrs_multi_gather_info(const scanrs_multi *mm, uint32_t *n_src, uint64_t *bounds, uint64_t *moved, uint64_t *host_bytes);
/* the same plan on the host, no device: from the source's global indptr (n_outer + 1), its bounds (n_src + 1) and the list:
 * out_indptr (n_idx + 1: the selected matrix's), bounds (n_dst + 1) and moved (n_src x n_dst). Any output may be NULL. */
int scanrs_host_plan_gather(const uint64_t *indptr, uint64_t n_outer, const uint64_t *src_bounds, uint32_t n_src,
                            const uint64_t *idx, uint64_t n_idx, uint32_t n_dst, uint64_t *out_indptr, uint64_t *bounds,
                            uint64_t *moved);

/* ---- to_adaptive of a whole scanrs_multi, in either orientation -----------
 * scanrs_mat_to_adaptive_major over the shards: the stored counts of the WHOLE matrix as one table of AdaptiveVec encodings, made on
 * the devices; only the encoded arenas (and, for INNER, 8 (n_inner + 1) bytes of indptr per shard) cross the host link. The export
 * owns one pair of host arenas per shard and ONE table in global order; scanrs_adaptive_export_info / _vecs / _free work on it
 * unchanged, kind_counts and total_bytes are over the whole table. Map and offset are ignored, as in scanrs_mat_to_adaptive.
 *
 * SCANRS_EXPORT_STORED: every shard encodes its own outer vectors on its own device and thread. outer_global vectors of
 * len = n_inner, under the scanrs_multi's storage flag; vector by vector and byte for byte scanrs_mat_to_adaptive of an unsharded
 * handle made from scanrs_multi_to_csmat.
 *
 * SCANRS_EXPORT_INNER, the inverse of scanrs_multi_create_adaptive_inner: one AdaptiveVec per INNER position (per gene, for a
 * cell-sharded genes x cells matrix), each spanning all shards: n_inner vectors of len = outer_global, the table
 * scanrs_mat_create_adaptive / scanrs_multi_create_adaptive_inner take with the OTHER storage flag. Byte for byte
 * scanrs_mat_to_adaptive of an unsharded handle made from the host-transposed whole triplet, whatever the number of shards and the
 * cut. An encoding cannot be concatenated from the shards' pieces (Dense3 packs 21 fields per word, S* has 256-index blocks,
 * choose_storage looks at the whole vector), so the vectors are made whole on a device first: (1) every shard settles its transposed
 * copy (kept by the handle, as a product would) and sends its indptr down; (2) the host plan (scanrs_host_plan_export) deals the
 * inner positions in n_shards contiguous slabs by nonzeros, slab d to shard d's device; (3) every destination assembles the CSR of
 * its slab over all outer_global positions, reading the sources' transposed copies in place (through the peer mapping where the
 * devices differ; peer access is enabled from every destination to every source), every index raised by the source's outer_begin;
 * (4) it encodes the slab, brings the two arenas down and releases the slab - 8 bytes per nonzero of the slab beside the encoder's
 * temporaries; a destination that cannot hold them returns SCANRS_ERR_DEVICE naming the shard and the bytes (a slab is not split
 * into rounds). Integer work without atomics: two calls return the same bytes.
 *
 * major outside 0..1, force_kind outside -1..7 and a null argument are SCANRS_ERR_ARGUMENT, before any device work. A matrix without
 * outer vectors, empty shards and empty slabs are valid. On any failure nothing is leaked and *out is NULL. Per shard,
 * scanrs_mat_get_counter "export_plan_us" / "export_pull_us" / "export_encode_us": wall clock of the phases of the last call.
 * Not served: the one-process-per-GPU forms (RCCL, host hook). Distinct devices: as for §7m / §7n, no run on several physical GPUs
 * has exercised the peer path yet. */
int scanrs_multi_to_adaptive(scanrs_multi *mm, int major, int force_kind, scanrs_adaptive_export **out);
/* What the multi call did: the shard count, slab_bounds (n_shards + 1: the table entries shard d encoded - INNER: the plan's slabs
 * of inner positions; STORED: the shards' own ranges), moved (n_shards x n_shards, source-major: moved[s * n_shards + d] = the
 * nonzeros of source shard s in slab d; STORED: the shards' nonzeros on the diagonal) and arena_bytes (per shard: the bytes of its
 * two arenas that crossed the host link). Any pointer may be NULL. SCANRS_ERR_ARGUMENT on an export that scanrs_multi_to_adaptive
 * did not make. */
int scanrs_adaptive_export_multi_info(const scanrs_adaptive_export *e, uint32_t *n_shards, uint64_t *slab_bounds, uint64_t *moved,
                                      uint64_t *arena_bytes);
/* The plan of SCANRS_EXPORT_INNER on the host, no device: counts (n_src x n_inner, source-major) = the stored entries source s holds
 * of every inner position; out_indptr (n_inner + 1) = the scan of the column sums, the whole matrix's inner-major indptr;
 * slab_bounds (n_dst + 1) = scanrs_plan_shards over it; moved (n_src x n_dst) = the entries of source s in slab d. Any output may be
 * NULL. n_src and n_dst outside 1 .. 16 and a null table with n_inner > 0 are SCANRS_ERR_ARGUMENT. */
int scanrs_host_plan_export(const uint64_t *counts, uint32_t n_src, uint64_t n_inner, uint32_t n_dst, uint64_t *out_indptr,
                            uint64_t *slab_bounds, uint64_t *moved);

/* ---- measurement ------------------------------------------------------------------------- */

/* Per-kernel-class HIP-event timing on the handle's stream (bench.py roofline leg). */
typedef struct {
    char name[48];
    uint64_t launches;
    double total_ms;
    double algorithmic_bytes;   /* summed over launches, SURVEY.md §8d accounting */
    double onchip_gather_bytes; /* panel bytes gathered through L2 / L1 by the sparse products (nnz * 8 * l), else 0 */
} scanrs_kernel_stat;
int scanrs_profile_enable(scanrs_mat *m, int on);
int scanrs_profile_reset(scanrs_mat *m);
/* Fills up to `cap` entries, writes the total count to *n. */
int scanrs_profile_get(scanrs_mat *m, scanrs_kernel_stat *out, uint32_t cap, uint32_t *n);
/* Which f64 product kernel serves this handle (and its views): 0 = auto (L2-blocked gather for large matrices and
 * panels of 16+ columns, plain gather otherwise), 1 = plain gather, 2 = L2-blocked gather, 3 = hybrid: LDS-staged panel
 * tiles over a tile-bucketed layout of the matrix plus the L2-blocked gather over the nonzeros that overflow it, run side
 * by side (panels of 16..104 columns; the layout is built on first use under a given map; other widths take path 2).
 * All are HIP kernels; results agree to rounding. */
int scanrs_mat_set_spmm_path(scanrs_mat *m, int path);
/* Tuning options of a handle (shared by its views); defaults are the measured optimum on MI355X.
 *   "tile_k" (2)        hybrid product: record positions per (outer vector, visit): 2, 3 or 4
 *   "tile_s" (32)       hybrid product: outer vectors per wave (32, or 28 with tile_k 2 or 4: 168 instead of 184 registers per tile wave)
 *   "ov_tile_kb" (0)    hybrid product: panel slice per step of the overflow gather (0 = twice l2_tile_kb)
 *   "tile_max_overflow" (0.35)  auto path: an orientation whose tile layout would leave more than this share of the nonzeros to
 *                       the overflow gather (dense outer vectors: genes detected in most cells) stays on the gather kernels
 *   "tile_ku" (1)       hybrid product, tile_k 2: 1 = one of the two positions takes only count-1 nonzeros, whose rows are added
 *                       without a weight (maps whose value at count 1 is an outer factor times an inner factor); 0 = none
 *   "tile_t" (48)       hybrid product: panel rows per tile (<= 24 tile_k)
 *   "tile_b" (4)        hybrid product: tile buffers in the LDS ring (tile_t * tile_b <= 192); a nonzero may wait tile_b - 2 visits
 *   "tile_auto" (1)     path 0 may use the hybrid product for matrices of 2^24+ nonzeros (layout built when svd_bk / svd_rand
 *                       start, or at the second product under the same map, if the device has room: ~12 B per nonzero)
 *   "tile_overlap" (1)  hybrid product: the overflow gather runs beside the tile kernel (0: after it; measurement only)
 *   "l2_tile_kb" (3584) panel slice per step of the L2-blocked gather
 *   "spmm_order" (1)    L2-blocked gather launch order: 0 storage order, 1 longest vectors first when a launch is a few
 *                       rounds of waves, 2 always longest first
 *   "hot_segment" (512) nonzeros per step from which a vector gets a whole workgroup (0 = never)
 *   "materialize" (1)   keep the values of the map prefix per nonzero on the copy with few, long outer vectors
 *   "slice_walk" (1)    Ix1 products / moments on the copy with few, long vectors stage the inner-indexed arrays in LDS slices
 *   "spmv_lds" (1)      Ix1 products on the copy with many short vectors stage the vector in LDS parts
 *   "overlap" (1)       small dense work of the solvers runs on a second stream beside the sparse passes
 *   "col_moments" (1)   mean_var_axis / sum of a log-normalized map (scale factors on the summed-over axis, then a logarithm):
 *                       walk the copy whose outer vectors are the summed-over axis — a table of the map at counts 1..8 per outer
 *                       vector instead of one logarithm per nonzero, sums scattered into LDS as 64-bit fixed point (order-
 *                       independent, so bit-reproducible). Taken when that copy exists and the matrix is large; 2: whenever
 *                       eligible; 0: never. Eligible is what scanrs_host_col_moments_plan accepts: then, for EVERY slice, sum and
 *                       mean are within 1e-12 relative of the exact values and the variance within 1e-10 S2/m (S2 = the slice's sum
 *                       of squares, m = the extent of the summed-over axis); every other map takes the ordinary pass.
 *   "device_factor" (1) svd_bk: the b x b Cholesky factors of CholeskyQR and the coefficient bookkeeping of qr(K) stay on the
 *                       device (no host round trip per orthonormalisation; falls back to the host path by itself when a
 *                       factorization does not converge within the queued passes); 0: host factorizations
 *   "d2h_threads" (4)   host threads that empty the pinned ring of a large result download
 *   "merge_fused" (1)   scanrs_merge_clusters: per-cell totals plus ONE grouped pass over the nonzeros per call (per gene-major tile of
 *                       1536 clusters), every candidate from those sums; 0: compute_sseq_params on the union and the pairwise DE for
 *                       every candidate, as the reference calls them (A/B and test baseline). Same labels; p-values agree to ~1e-12
 *   "sseq_grid_cap" (16384) workgroups of the sSeq group / moment pass and of its class walk at most (1 .. 16384). Results do not depend
 *                       on it; a small cap makes every wave take several genes or cells in turn, which tests use on small matrices
 *   "subset_scatter" (1) integer sums over a column list (scanrs_mat_sum_rows_u64, _sum_cols_u64, _sum_rows_dual_u64) whose result axis is
 *                       the outer dimension of a copy that does not exist yet: 1 = scattered into the result with 64-bit integer atomics
 *                       from the copy that exists (exact in any order; no transposed copy is built); 0 = the missing copy is built
 *                       and walked without atomics. Same results.
 *   "tile_spare_cus" (1) the persistent tile kernel launches as many workgroups as its number of item rounds needs (3 977 equal items:
 *                       16 rounds on 256 workgroups and on 249); the CUs left over serve the side streams during the pass (0: one per CU)
 *   "spmv_row_table" (1) Ix1 products over many short outer vectors (IRLBA's A v on the cell-major copy): a map that depends on the count
 *                       and the outer position alone is looked up by count from a table made per vector (0: values materialized per nonzero)
 *   "gemm_direct" (1)   dense panel products X W read their operands straight from memory into the MFMA registers
 *                       (0: the LDS-tiled kernels)
 *   "reuse_cmax" (1e5)  svd_bk: coefficient bound above which a projection column is recomputed directly
 *   "side_build" (1)    scanrs_normalize starts a helper thread (own stream) that builds what the PCA behind it needs: the first
 *                       product's tile layout, the transposed copy of the matrix and the second orientation's layout, in that
 *                       order, beside the normalisation passes and the solver's first product (a solver called without a
 *                       normalize before it starts the helper for the second orientation itself); 2: the helper starts behind
 *                       the normalisation passes instead of beside them (measured the same); 0: everything is built on demand by
 *                       the calling thread
 *   "tile_split" (1)    tile layout (default tile shape): an outer vector owns as many SLOTS (units of tile_k record positions per visit)
 *                       as its density asks for: V = round(x / tile_split_x), at least 1, at most 32, x = its expected nonzeros per
 *                       panel tile; its nonzeros are dealt to its slots round-robin; below tile_split_min it owns none and all of it
 *                       goes to the overflow part. Makes the layout fit real count matrices (a few thousand genes detected in most
 *                       cells, most genes in almost none). 0: one slot per vector
 *   "tile_split_x" (1.8), "tile_split_min" (0.5)   the two densities of that rule, in nonzeros per tile
 *   "tile_build_one_pass" (1)  the wave-level layout builder writes the records and collects the nonzeros without a position in ONE
 *                       walk over the matrix (temporaries of 8 bytes per nonzero, then a compaction); 0: a counting walk first
 *   "tile_weights_wide" (1)  the weight refresh of a unit-mode layout works four positions per thread with wide loads and stores
 *                       (0: one position per thread; same values)
 *   "dense_side_no_lds" (0)  experiment: dense kernels queued on the side streams use the register-only MFMA forms, which can run
 *                       beside the persistent tile kernel (measured slower: DESIGN.md section 9)
 *   "tile_dense" (1)    tile layout of the default shape: 1 = DENSE record streams — the records of a (wave, visit) are a packed list,
 *                       as long as the most loaded of the item's 8 waves needs for the tile that leaves the ring, and the accumulator of
 *                       a record is selected at run time (VGPR index mode): about 1.05 record positions per nonzero and no overflow
 *                       beyond the vectors too sparse to own a slot; 0 = the round-4 form, tile_k fixed positions per (slot, visit)
 *   "tile_sort_slots" (2)  dense tile layout: 2 = the slots, sorted by load, are DEALT over the waves' groups (rank k -> group k mod n, accumulator
 *                       k div n): every group holds one slot of every load stratum, so the 8 waves of an item carry the same number of records
 *                       per visit AND all items of a part move through the panel's tiles at the same pace (a tile stays in L2 between the
 *                       first and the last workgroup that stages it: gene-major pass 15.5 -> 13.7 ms); 1 = 32 consecutive ranks per group
 *                       (rounds 5-6: equal waves, but items of very different load); 0 = vector order
 *   "tile_one_walk" (1)  dense tile layout: 1 = built in ONE walk over the matrix (the (group, part) blocks of the tile-sorted record
 *                       list start at the prefix sums of their capacities, found by binary searches; counts above 15 leave through
 *                       a bounded list); 0 = a counting walk and a filling walk. The same layout bit for bit.
 *   "tile_fold" (1)     dense tile layout under a map whose count-1 value is a product of a per-row and a per-column factor (every
 *                       normalisation of the reference): 1 = the weight of a record position holds only the factor of the side that owns
 *                       the logarithm (with the count's ratio); the other side's factor rides in the staged panel (columns of the
 *                       product's inner side) or is applied when a vector's sums are collected (outer side) - one table lookup per
 *                       position in the weight refresh instead of two; 0 = both factors in every weight. Same products to rounding.
 *   "tile_wtab" (1)     dense tile layout under such a map (with tile_fold 1): 1 = the product kernel evaluates the map itself - it gathers a
 *                       record position's weight from a table of 16 entries by count per place of the layout (or per inner position),
 *                       addressed by the record's own count and slot / ring row; no per-position weight exists in memory and a normalize
 *                       rewrites only the table. Counts above 15 are served by the overflow part, where the chain is evaluated per
 *                       nonzero. 0 = one f64 weight per record position, rewritten by every normalize (the form every other map takes)
 *   "tile_big_list_cap" (0)  dense tile layout, one-walk build: entries of the list that carries the nonzeros with counts above 15 to the
 *                       overflow part (0: max(4 M, nnz / 64)); a matrix with more of them is built by the two-walk form instead.
 *   "tile_emit_staged" (1)  dense tile layout, diagnostic: 0 makes the emission of the record streams search its per-visit tables in global
 *                       memory instead of LDS - the form taken by itself when a part has more than 4 000 tiles. Same layout.
 *   "tile_poison_slack" (0)  test hook: 1 = the rows behind the end of the tile kernel's compact panel copy (the slack its staging may
 *                       read, never an index or record array) are filled with NaN before every tile kernel launch. Same products bit for bit.
 *   "tile_builder" (1)  1: wave-level builder of the tile layout (default tile shape); 0: per-thread walk (reference form)
 *   "tile_build_waves" (0)   cap on the waves per CU of that builder (0: as many as fit)
 *   "sync_timeout_s" (120)  PROCESS-WIDE (same as scanrs_set_global_option): deadline of every host-side wait for the device
 * Unknown keys return SCANRS_ERR_ARGUMENT. The only environment variables the library reads are the diagnostics
 * SCANRS_TRACE and SCANRS_TRACE_EIG (phase timings on stderr). */
int scanrs_mat_set_option(scanrs_mat *m, const char *key, double value);
/* Event counters of the handle (diagnostics): "bk_host_retries" = svd_bk calls whose device-side factorizations did not
 * converge within the queued passes and that were run again with host factorizations. The decisions of the last svd_bk on the
 * handle about its reused projection (host-side stores; a retry on the host path overwrites them with its own): "bk_q" / "bk_b" =
 * columns of the Krylov basis and of one block; "bk_coef_valid" = 1 when the coefficient bookkeeping Q = K C held (no panel was
 * completed with random directions); "bk_flagged_older" = columns of the blocks before the last whose max |C| reaches "reuse_cmax",
 * counted before any raise; "bk_limit_branch" = 0 none flagged, 1 they fit the repair pass, 2 bound raised to the largest flagged,
 * 3 raised to the largest that has to stay dense, 4 bound unchanged and a pass wider than 104 columns; "bk_limit_bits" = the f64 bit
 * pattern of the bound finally used; "bk_direct_columns" = columns recomputed by a sparse product (the last block included when
 * "bk_last_direct" is 1); "bk_full_direct" = 1 when the whole projection was one sparse product of Q; "bk_early_projections" = dense
 * projections queued beside the iterations; "bk_cmax_dense_bits" = f64 bits of the largest max |C| among the columns that took the
 * dense route (0.0 when none did). First-call accounting, host microseconds of
 * the calling thread since the handle was made: "t_layout_us" (tile layout builds), "t_side_wait_us" (waiting for the helper
 * thread of "side_build"), "t_start_panel_us", "t_delivery_us" (U, V to host arrays); process-wide: "t_alloc_us" / "alloc_calls"
 * (hipMalloc). The tile layouts of the handle (both orientations, summed): "tile_positions" = record positions the tile kernel works
 * per pair of passes, "tile_served_nonzeros" = nonzeros among them (the rest is padding), "tile_overflow_nonzeros" = nonzeros left
 * to the overflow gather. "partition_rounds" = rounds of the last scanrs_mat_partition_on_thresholds on this handle, the final round
 * that changes nothing included; "partition_allreduces" = the exchange steps of the last scanrs_mat_partition_on_thresholds_sharded
 * (0 on an unsharded handle). "de_pairs_passes" / "de_pairs_literal" = the last scanrs_sseq_de_pairs[_sharded] on this handle: its passes over
 * the nonzeros and its pairs on the literal route. "de_shard_tests" / "de_shard_allreduces" = the last sSeq DE call (scanrs_sseq_de_pairs_sharded,
 * scanrs_merge_clusters_sharded and scanrs_cluster_medoids_sharded included) on this handle: the
 * tests this rank launched on the device, and the exchange steps of a sharded handle (0 on an unsharded one). "subset_masked_passes" / "subset_scatter_passes" = sums over a column list made on
 * this handle so far: from the copy whose outer dimension is the result axis (masked walk or listed vectors, no atomics) / through the
 * integer scatter from the other copy ("subset_scatter"); "subset_allreduces" = the exchange steps of the last
 * scanrs_mat_sum_rows_u64_sharded or kin on this handle (0 on an unsharded one). "regather_plan_us" / "regather_pull_us" /
 * "regather_finish_us" = on a shard made by scanrs_multi_gather_outer / scanrs_multi_rebalance, the wall clock of the plan (one phase,
 * the same on every shard) and of the shard's own thread in pull and finish. "export_plan_us" / "export_pull_us" /
 * "export_encode_us" = on a shard of a scanrs_multi, the last scanrs_multi_to_adaptive: the wall clock of the plan (the transposed
 * copies, their indptr to the host and the host plan: one phase, the same on every shard; 0 for SCANRS_EXPORT_STORED) and of the
 * shard's own thread in the pull of its slab (0 for STORED) and in encode + download. "reshard_upload_us" / "reshard_count_us" /
 * "reshard_split_us" / "reshard_exchange_us" / "reshard_transpose_us" = on a shard made by an inner-sharding constructor
 * (scanrs_multi_create_inner and kin), the wall clock of its thread in the phases upload, count (validation and the histogram),
 * split, exchange and transpose.
 * "transpose_route" = the sort the handle's transposed copy was built through (scanrs_host_transpose_plan gives the same decision
 * on the host): 0 no transposed copy built yet, or one without nonzeros; 1 one packed 64-bit key per nonzero; 2 the pair sort.
 * The route of the LAST sparse product A X on this handle (host-side stores, overwritten by every product; a solver's last pass):
 * "spmm_route" = its kernel family, one of SCANRS_SPMM_* below; "spmm_form" = the form within the family -
 *   tiles:               bit 0 dense records (0: fixed positions), bit 1 unit mode (0: the weighted kernel), bits 2-3 where a
 *                        position's weight comes from: 0 the weight stream, 1 the table by place, 2 the table by inner position;
 *                        bits 4-5 the factor kept out of the weights: 0 none, 1 the inner side's (it rides in the staged panel),
 *                        2 the outer side's (applied to the finished sums)
 *   spmv_lds:            0 the map evaluated per nonzero, 1 materialized values, 2 a table per row
 *   slice_walk, spmv2d:  bit 0 materialized values are read, bit 1 the first link's scale is interleaved with the vector (spmv2d),
 *                        bit 2 that scale is staged in LDS beside the vector (slice_walk)
 *   every other family:  0
 * "spmm_chunks" = the column chunks the panel went through in (1 outside the tile route), with SCANRS_SPMM_SLIVER set when a last
 * chunk under 16 columns went to the plain gather instead. */
#define SCANRS_SPMM_TILES 1        /* hybrid: LDS-staged tiles + gather of the overflow part */
#define SCANRS_SPMM_GATHER2D 2     /* L2-blocked gather */
#define SCANRS_SPMM_GATHER2D_F32 3 /* ... over an f32 copy of the panel (panel precision 1) */
#define SCANRS_SPMM_SLICE_WALK 4   /* 1 column, few long outer vectors: the vector in LDS slices */
#define SCANRS_SPMM_SPMV2D 5       /* 1 or 2 columns, a vector beyond L2: walked in 2 MB slices */
#define SCANRS_SPMM_SPMV_LDS 6     /* 1 column, many outer vectors: the vector in LDS parts */
#define SCANRS_SPMM_SPMV 7         /* 1 or 2 columns, a wave per item */
#define SCANRS_SPMM_GATHER 8       /* plain gather */
#define SCANRS_SPMM_SLIVER (1u << 16)
int scanrs_mat_get_counter(scanrs_mat *m, const char *key, uint64_t *value);
/* Process-wide options of the entry points that take no handle:
 *   "h5_threads" (8)               threads that inflate the chunks of a large filtered HDF5 read
 *   "eig_threads" (4)              host team of the Rayleigh-Ritz eigensolver for matrices of 768+ rows (1, 2 or 4)
 *   "knn_exhaustive" (0)           1: never use the bf16-MFMA filter of scanrs_knn*
 *   "knn_filter_min_points" (32768), "knn_ratio" (4), "knn_stats" (0)   tuning / statistics of that filter (the figures
 *                                  "knn_stats" prints are also returned by scanrs_debug_knn_last_stats)
 *   "knn_block_rows" (262144)      rows of the point set that scanrs_knn_sharded exchanges and searches at a time (at most
 *                                  256 MiB of exchange buffer at d = 128; the result does not depend on it)
 *   "sync_timeout_s" (120)         BOUNDED WAITS: no call of this library blocks on the device without a deadline. Every wait for
 *                                  a stream or an event (and every barrier between the shard threads of scanrs_multi_*) is a poll
 *                                  with this deadline in seconds; when it passes, the call returns SCANRS_ERR_DEVICE and
 *                                  scanrs_last_error() names the wait (function, file:line), the calling thread's last solver
 *                                  stages and which of the handle's streams (main / aux / aux2 / overflow) still had work; the
 *                                  same report and the whole stage ring go to stderr. Copies that were queued may still run: the
 *                                  host buffers given to the failing call (and the device's view of the handle) must not be
 *                                  reused or freed before the process exits. The handle must then be freed (its queued
 *                                  work never finished); start over in a fresh process — a process whose device stopped
 *                                  answering cannot be repaired from inside, and must not exec() another program either.
 *   (a value that is not finite is refused; "h5_threads", "eig_threads" and "knn_block_rows" below 1, "knn_ratio" below 2 and
 *   "knn_filter_min_points" below 0 are raised to that bound)
 *   "device_cache_fraction" (0.5)  device blocks of 1 MB and more that the library releases are kept for its next allocation of about
 *                                  their size, up to this share of the device's memory, instead of going back to the driver (VRAM
 *                                  that was just freed is scrubbed in the background; an allocation that lands on it waits:
 *                                  seconds for the tens of GB of a handle). 0: no cache. See scanrs_release_cached_memory. */
int scanrs_set_global_option(const char *key, double value);
/* Optional: loads the library's device code, starts the one-off host-side table computation of the seeded start panels, pins the
 * 72 MB host staging buffer a PCA's result delivery and start panel go through (kept in a process-wide pool across handles) and
 * touches the runtime paths the first call would otherwise initialise (~30-60 ms on MI355X): call it at program start to
 * keep that out of the first scanrs_mat_create / normalize / PCA. Everything works without it. */
int scanrs_init(void);
/* Optional: one allocation of `bytes` made now, on the calling thread's current device, from which the library carves its later
 * large buffers (about 70 bytes per nonzero for a matrix that goes through normalize + PCA with the hybrid product). A caller who
 * knows the size of the matrix before it is loaded takes the allocation's latency — on a device whose memory was just freed by
 * another process the driver is still scrubbing it, and an allocation waits for that — out of the first PCA. The reserve is an
 * arena: blocks carved from it return to it when the work queued before their release has run, neighbouring holes merge, and a
 * later request of any size is carved from them again; the reserve itself goes back to the driver with
 * scanrs_release_cached_memory once none of it is in use. */
int scanrs_reserve_device_memory(uint64_t bytes);
/* Gives the cached device blocks (see "device_cache_fraction") back to the driver / reports how much is cached on the calling
 * thread's current device. */
int scanrs_release_cached_memory(void);
int scanrs_cached_memory_bytes(uint64_t *bytes);
/* Device memory in the library's buffers right now, all handles of the process (blocks waiting in the cache not counted). */
int scanrs_device_memory_in_use(uint64_t *bytes);
/* Arithmetic of the large sparse products: 0 (default) = f64 throughout, the reference's arithmetic; 1 = opt-in fast
 * mode: the dense panel is rounded to f32 before it is gathered (half the on-chip bytes per nonzero), products and
 * sums stay f64. Singular values / loadings then agree with the f64 path to ~1e-7 relative, not to rounding. */
int scanrs_mat_set_panel_precision(scanrs_mat *m, int precision);
/* Block until all work queued on the handle's stream is done. */
int scanrs_mat_sync(scanrs_mat *m);

/* One pass of the factor step of the device-side CholeskyQR (`.qr()` of a b-wide panel, bk_svd.rs:94,98,123,127): g is the
 * n x n Gram matrix of the panel (row-major, n <= 128), `rows` the panel's row count (shift rule), `pass` the pass number
 * (from pass 1 on the step first tests max |g - I| < 5e-14 sqrt(n) and answers "converged"). rinv receives R^-1 with
 * g (+ shift I) = R^T R — or the identity when the step has nothing to apply. done: 1 converged or failed; status: 0 ok,
 * 1 Cholesky failed after 12 shifts, 2 non-finite input; err = max |g - I|; shift = diagonal shift used. For tests. */
int scanrs_mat_chol_rinv(scanrs_mat *m, const double *g, uint32_t n, uint64_t rows, int pass, double *rinv, int *done, int *status,
                         double *err, double *shift);

/* ---- the dense f64-MFMA products, one kernel at a time. For tests. ------------------------------------------------------------
 * The solvers reach the Gram kernels (C = X^T Y) and the GEMM kernels (Out = beta Cin + alpha X W) through two dispatchers that
 * pick a kernel from the shape; these entry points run one product on host arrays and can force the kernel. Routes: */
#define SCANRS_DENSE_GRAM_WAVE 1       /* one wave per 32 x 32 tile of C */
#define SCANRS_DENSE_GRAM_VEC 2        /* one vector (m = 1) against at most 128 columns, streaming */
#define SCANRS_DENSE_GRAM_TILED 3      /* 128 x 128 LDS tiles; symmetric form when Y is X */
#define SCANRS_DENSE_GEMM_WAVE 1       /* one wave per 16 rows x 16 / 32 / 64 columns */
#define SCANRS_DENSE_GEMM_TILED 2      /* 128 x 128 LDS tiles */
#define SCANRS_DENSE_GEMM_SKINNY_LDS 3 /* 256 x 64 LDS tiles */
#define SCANRS_DENSE_GEMM_DIRECT 4     /* operands straight from memory, W transposed and zero-padded first */
/* What the dispatcher would choose (host only, no device needed). kind 0: Gram of X (rows x n, ld ldx) and Y (rows x m, ld ldy),
 * flag = a skip flag is set (a queued orthonormalisation). kind 1: GEMM X (rows x n, ld ldx) times W (n x m), ldy ignored,
 * x_aligned16 = X starts on a 16-byte boundary, flag = the handle's "gemm_direct" option; odd ldx answers SCANRS_ERR_ARGUMENT as
 * the dispatcher does. side != 0: queued on a side stream under "dense_side_no_lds". *nt: 16-column MFMA tiles per wave (GEMM_WAVE:
 * 1, 2 or 4; GEMM_DIRECT: 1..7; else 0); *groups: column groups of the GEMM launch (Gram: 0). */
int scanrs_debug_dense_route(int kind, uint32_t n, uint32_t m, uint64_t rows, uint32_t ldx, uint32_t ldy, int x_aligned16, int side,
                             int flag, int *route, uint32_t *nt, uint32_t *groups);
/* C (n x mcols, ld = mcols; read first, so that what the kernels leave untouched keeps the caller's values) = X^T Y over `rows` rows.
 * x: rows_alloc x ldx, y: rows_alloc x ldy host arrays, uploaded whole (rows_alloc >= rows: the surplus rows are there for the kernels
 * not to read). y == NULL: Y is X itself, the same device pointer (needs mcols == n, ldy == ldx). route 0: the dispatcher's choice;
 * else that kernel, or SCANRS_ERR_ARGUMENT when its own preconditions fail (GRAM_VEC: mcols == 1, n <= 128, no skip; GRAM_TILED: even
 * ldx, ldy). skip != 0: the call runs with the handle's skip flag pointing at a device int that holds 1. */
int scanrs_debug_dense_gram(scanrs_mat *m, int route, const double *x, uint32_t ldx, uint32_t n, const double *y, uint32_t ldy,
                            uint32_t mcols, uint64_t rows, uint64_t rows_alloc, int skip, double *c);
/* out (rows_alloc x ldo; read first, written back whole) = beta cin + alpha X W. x: rows_alloc x ldx (even), w: n x ldw,
 * cin: rows_alloc x ldc or NULL (then beta must be 0). x_skew 0 / 1: X's device base is moved by that many doubles inside its
 * allocation (1: not 16-byte aligned). in_place: Cin is the device buffer of Out (ldc == ldo; cin ignored). route as above
 * (GEMM_DIRECT: X aligned, n >= 16, rows >= 64, mcols <= 4096). The host arrays x and out must not overlap. */
int scanrs_debug_dense_gemm(scanrs_mat *m, int route, const double *x, int x_skew, uint32_t ldx, uint32_t n, const double *w, uint32_t ldw,
                            uint32_t mcols, uint64_t rows, uint64_t rows_alloc, double alpha, double beta, const double *cin, uint32_t ldc,
                            double *out, uint32_t ldo, int in_place, int skip);
/* w (rank x ldw; read first, written back whole) = B^T X with b: n x rank, x: n x ldx (ldx even, >= l rounded up to even). xc (n x ldc,
 * or NULL; needs l and ldc even): the compact copy of X's first l columns the same kernel writes; read first, written back whole. */
int scanrs_debug_weighted_colsum(scanrs_mat *m, const double *b, uint32_t rank, const double *x, uint32_t ldx, uint64_t n, uint32_t l,
                                 double *w, uint32_t ldw, double *xc, uint32_t ldc);

/* ---- the bf16-MFMA filter of scanrs_knn* / scanrs_find_nn (knn.hip). For tests. -------------------------------------------------
 * The filtered search (default from "knn_filter_min_points" points on, d <= 58, k <= 64, at least 256 queries, max |coordinate|
 * inside the magnitude window and every coordinate finite) promises the result of the exhaustive f64 kernel: per round, a query's
 * candidate list must hold every point whose f64 distance is <= the query's threshold tau, and little else.
 * scanrs_debug_knn_filter runs the operand preparation, the threshold kernel and ONE pass of the filter kernel, the kernels
 * the search itself launches, on host arrays: queries n_q x d, points n_p x d (row-major), tau[n_q] (squared distances; +inf =
 * everything passes), over rows 0, stride, 2 stride, ... of the points. cnt[n_q]: candidates found (a value > cap: the list
 * overflowed and the search would redo that query exhaustively); cand[n_q x cap]: the lists, row indices of `points` in no
 * particular order, slots that were not written = UINT32_MAX. SCANRS_ERR_ARGUMENT when d > 58 or the input is outside the window. */
int scanrs_debug_knn_filter(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, const double *tau,
                            uint64_t stride, uint32_t *cnt, uint32_t *cand);
/* What the last scanrs_knn / scanrs_knn_device / scanrs_find_nn of the process did (no device needed). *filtered: 1 = it went
 * through the filter; then *first_stride = the stride of the subset ranked exactly first and *n_rounds filter rounds followed, of
 * which the first `capacity` are reported: strides[i], points[i] = points of that subset, cand_sum[i] / cand_max[i] = sum and
 * maximum of the candidate counters over the queries (an overflowed list counts with what its counter reached), overflowed[i] =
 * queries redone exhaustively. Not filtered: *n_rounds = 0. The "knn_stats" option prints the same figures on stderr. */
int scanrs_debug_knn_last_stats(int *filtered, uint64_t *first_stride, uint32_t *n_rounds, uint32_t capacity, uint64_t *strides,
                                uint64_t *points, uint64_t *cand_sum, uint32_t *cand_max, uint32_t *overflowed);
/* The filter's constants (host only): the margin gamma, the list capacity, the largest d and k and the smallest query count it
 * takes, and the magnitude window coord_min <= max |coordinate| <= coord_max outside of which the exhaustive kernel answers. */
int scanrs_debug_knn_filter_params(double *gamma, uint32_t *cap, uint32_t *dmax, uint32_t *k_max, uint64_t *nq_min, double *coord_min,
                                   double *coord_max);

/* Diagnostics of the bounded waits (no device needed): runs the library's wait loop on an event that is never signalled and
 * returns SCANRS_ERR_DEVICE once `timeout_s` seconds have passed, with the report a real stuck wait leaves behind. */
int scanrs_debug_wait_never(double timeout_s);
/* ... and the barrier between the shard threads of the single-process multi-GPU form, entered by one thread of `world` alone */
int scanrs_debug_barrier_alone(uint32_t world);
/* ... and the bookkeeping of a reserve made by scanrs_reserve_device_memory (no device needed: the arena is driven on a made-up address
 * range): `rounds` random rounds of carving and giving back blocks; SCANRS_OK when no two live blocks ever overlapped, every block
 * stayed inside the range, neighbouring holes always merged and the arena was whole again at the end. */
int scanrs_debug_arena_selftest(uint32_t rounds, uint64_t seed);

/* ---- host-side dense helpers (no device needed; used by the solvers where the reference calls
 * LAPACK on k x k matrices, exposed so the CPU test-suite can check them) ------------------------- */
/* in place upper Cholesky G = R^T R (row-major n x n); SCANRS_ERR_NUMERICAL when G is not SPD */
int scanrs_host_chol_upper(double *g, int n);
/* in place inverse of an upper-triangular matrix */
int scanrs_host_inv_upper(double *r, int n);
/* symmetric eigen-decomposition, w descending, z[i*n + j] = component i of eigenvector j */
int scanrs_host_sym_eig(const double *a, int n, double *w, double *z);
/* the k leading eigenpairs only: w[0..k) descending, z row-major n x k */
int scanrs_host_sym_eig_topk(const double *a, int n, int k, double *w, double *z);

/* ---- sSeq differential expression (diff-exp/src/diff_exp.rs, dist.rs; NbExactBackend::LogSpace and ::Ratio) ----------------
 * Rows of the handle are genes and columns are cells (the reference's feature x barcode matrix; use scanrs_mat_t on a cell-major
 * handle). DE reads the stored u32 counts and ignores the handle's map and offset. Labels are one int16 per cell: the group
 * 0 .. n_groups - 1 (n_groups <= 8192) or -1 for a cell in no group. Outputs of
 * several tests are row-major genes x n_tests arrays. Checkpoints of `snoop`: 0.0, 0.1, 0.6, 0.75, 0.9, 0.95, 1.0
 * (diff_exp.rs:137-300); a set cancel flag returns SCANRS_ERR_CANCELLED.
 *
 * Sharded handles (scanrs_mat_set_shard[_comm], the shards of scanrs_multi_*). scanrs_sseq_params, scanrs_mat_group_sums,
 * scanrs_sseq_de and scanrs_sseq_de_backend (modes 0, 1 and 2, both backends) serve a handle whose CELLS - the view's columns - are
 * the sharded dimension: a genes x cells CSC handle, or scanrs_mat_t of a cells x genes CSR one. A handle sharded over the genes
 * returns SCANRS_ERR_ARGUMENT. On a sharded handle every per-cell argument and output spans the WHOLE matrix, not the local slice:
 * labels, size_factors (input and output) and umi_counts have outer_global entries (umi_counts one per selected cell) and
 * cell_indices holds global indices. Every rank passes the same values and receives the same complete outputs; each rank uploads
 * only its slice [outer_begin, outer_begin + local columns) to the device. Every output equals the call on one unsharded handle of
 * the whole matrix bit for bit, for any number of shards and any transport: all sums that cross the shards are integers and travel
 * as u64 sum all-reduces (dtype 1 of scanrs_allreduce_fn; no floating-point all-reduce is used) - the per-cell totals
 * (outer_global u64 of device scratch per rank), the largest count, the group sums, and the 128-bit fixed-point moments as 32-bit
 * limbs - and the host folds (median, size-factor sums) run replicated over the global arrays in cell order. The tests are split
 * over the ranks by gene, rank r launching those of genes [G r / W, G (r + 1) / W), and their p-values are gathered by one more u64
 * all-reduce over the bit patterns; BH, log2 fold change and the means are replicated. Every rank polls its `snoop` at the same
 * checkpoints and must see the same cancel flag; scanrs_multi_sseq_de lets only shard 0 report progress. Counters
 * (scanrs_mat_get_counter): "de_shard_tests" = the tests this rank launched on the device in the last DE call (an unsharded
 * handle: all of them), "de_shard_allreduces" = the exchange steps of the last params / group sums / DE call.
 * What stays refused on a sharded handle (SCANRS_ERR_ARGUMENT, "sharded" in scanrs_last_error()) are the PLAIN calls
 * scanrs_sseq_de_pairs, scanrs_merge_clusters and the statistics over a column list (scanrs_mat_sum_rows_u64 and its kin). All of
 * them are served through collective entry points of their own: scanrs_sseq_de_pairs_sharded, scanrs_merge_clusters_sharded and
 * scanrs_mat_sum_rows_u64_sharded ... scanrs_mat_mean_var_rows_sharded (declared beside them). */

/* `compute_sseq_params` (diff_exp.rs:458-500). cell_indices (n_sel entries, or NULL for every cell): only those cells get a
 * size factor, the rest 0. umi_counts (one per selected cell, or NULL): replaces the per-cell totals. Size factors are the
 * totals over their interpolated median (stat.rs:116). Outputs: size_factors (cols), gene_means, gene_variances, use_genes,
 * gene_moment_phi, gene_phi (rows each), zeta_hat and delta (one each).
 * The moments. Σ x/sf_c and Σ (x/sf_c)² are exact integer sums of the f64 terms, each rounded once to a power-of-two quantum
 * (128-bit fixed point: no floating-point atomics, the same bits from either copy, any arrival order and any sharding). For EVERY
 * gene the mean is within 1e-12 of its exact value relative and the variance within 1e-10 S2 / m absolute (S2 the gene's own
 * Σ (x/sf_c)², m the number of selected cells), whatever the spread of the counts and of the size factors (terms x/sf_c between
 * 2^-440 and 2^440). One quantum serves all genes - chosen from the bound m max_count max(1/sf) of the largest sum - when a count
 * of 1 under the largest factor keeps 40 bits of its own below it, and 33 bits of its square below the second sum's; otherwise one
 * more walk over the nonzeros finds every gene's largest term (an integer maximum; on a sharded handle one more u64 all-reduce of
 * genes x world entries) and every gene is rounded to a quantum of its own. tests/test_gpu_sseq_moments.py holds this to exact
 * rational sums. */
int scanrs_sseq_params(scanrs_mat *m, double zeta_quintile, const uint64_t *cell_indices, uint64_t n_sel, const double *umi_counts,
                       double *size_factors, double *gene_means, double *gene_variances, uint8_t *use_genes, double *gene_moment_phi,
                       double *zeta_hat, double *delta, double *gene_phi);
/* `sseq_params_from_moments` (diff_exp.rs:377-456), host only: n entries of mean_g / var_g; n_genes drives the (G-1), (G-2)
 * denominators of delta. */
int scanrs_sseq_params_from_moments(const double *mean_g, const double *var_g, uint64_t n, double sum_size_factors, double n_cells,
                                    double n_genes, double zeta_quintile, uint8_t *use_genes, double *gene_moment_phi, double *zeta_hat,
                                    double *delta, double *gene_phi);
/* one pass over the nonzeros: sums[gene * n_groups + group] of the counts (u64, exact); cells_per_group (may be NULL) */
int scanrs_mat_group_sums(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, uint64_t *sums, uint64_t *cells_per_group);
/* `sseq_differential_expression` (diff_exp.rs:122-175) from labels. mode 0: each group against all other labelled cells
 * (n_tests = n_groups; Cell Ranger's per-cluster DE, utils.rs:77-117); mode 1: group 0 against group 1 (n_tests = 1).
 * size_factors (cols), gene_means, gene_phi, use_genes (rows): the SSeqParams fields. A side's size factor is the sum of
 * size_factors over its cells. Outputs (rows x n_tests): the DiffExpResult fields sums_in, sums_out, p_values,
 * adjusted_p_values, log2_fold_change, normalized_mean_in, normalized_mean_out. */
int scanrs_sseq_de(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, int mode, const double *size_factors, const double *gene_means,
                   const double *gene_phi, const uint8_t *use_genes, uint64_t big_count, const scanrs_snoop *snoop, uint64_t *sums_in,
                   uint64_t *sums_out, double *p, double *p_adj, double *log2fc, double *mean_in, double *mean_out);
/* `sseq_de_from_sums` (diff_exp.rs:177-300) on the device: sums_a / sums_b (n_genes x n_tests), the sides' size factors
 * sf_a / sf_b (n_tests each). Needs a gfx950 device. Checkpoints 0.75 .. 1.0 only. */
int scanrs_sseq_de_from_sums(uint64_t n_genes, uint32_t n_tests, const uint64_t *sums_a, const uint64_t *sums_b, const double *sf_a,
                             const double *sf_b, const double *gene_means, const double *gene_phi, const uint8_t *use_genes,
                             uint64_t big_count, const scanrs_snoop *snoop, double *p, double *p_adj, double *log2fc, double *mean_in,
                             double *mean_out);
/* `NbExactBackend` (dist.rs:52-68): the kernel of the exact branch. LogSpace is the log-sum-exp over per-term lnΓ values; Ratio is
 * the mode-anchored ratio recurrence `nb_exact_test_ratio` (dist.rs:116-215): one division and a few multiplies per term. */
enum { SCANRS_NB_EXACT_LOGSPACE = 0, SCANRS_NB_EXACT_RATIO = 1 };
/* `sseq_differential_expression_with_cancellation_backend` (diff_exp.rs:125-161) from labels: scanrs_sseq_de with the exact
 * test's backend; any other value of `backend` returns SCANRS_ERR_ARGUMENT. scanrs_sseq_de is this call with LogSpace.
 * It also takes mode 2, the shared-control shape: every group 1 .. n_groups-1 against group 0 (n_tests = n_groups - 1, test j
 * is group j + 1 as side a and group 0 as side b; needs n_groups >= 2). The control's sums and size factor are computed once;
 * every test equals the mode 1 call of its two groups bit for bit. (scanrs_sseq_de refuses mode 2.)
 * Ratio on the device differs from dist.rs:199-203 in one deliberate way: the reference falls back to LogSpace only when the
 * observed term U[x_a] is 0 or not finite; here a test whose U[x_a] is not finite or below 2^-970 falls back, in the same call,
 * and gets exactly the p-value that backend = LogSpace gives it. For 0 < U[x_a] < 2^-970 the terms at and below U[x_a] sink
 * into the denormals and the serial partition loses its bits (at U[x_a] = 4.9e-324 the serial restatement returns 5.9e-323
 * where LogSpace returns 0). Elsewhere the device sums the reference's terms in a fixed tree rather than serially.
 * Both backends differ from the reference in one more deliberate way, on the device and in the host forms below. With
 * sf_a / phi == sf_b / phi bit for bit the terms k and n - k are equal in exact arithmetic, so the mirror n - x_a of the observed
 * term belongs to the extreme set; the reference leaves that to `<=` on two differently rounded numbers and loses the mirror in
 * some cases (measured on its formulas in double precision: (x_a, x_b, sf, mu, phi) = (30, 2000, 50, 20, 0.5) LogSpace 4.86e-89
 * for 7.83e-89; (450, 440, 5e5, 1e-3, 0.13) Ratio 0.7377 for 0.7629; (120, 80, 7, 10, 0.3) Ratio 0.2175 for 0.2292). Here LogSpace
 * forms a term as the sum of one number per side, which the mirror term adds in the other order (the same bits), and Ratio takes
 * the mirror term by its index. LogSpace also takes ln Gamma(sf/phi + k) - ln Gamma(sf/phi) as one quantity (no cancellation of
 * two values of size (sf/phi) ln(sf/phi)); at sf/phi = 2e8 the reference's formula in double precision is off by 1e-7 to 2e-6 of p. */
int scanrs_sseq_de_backend(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, int mode, const double *size_factors,
                           const double *gene_means, const double *gene_phi, const uint8_t *use_genes, uint64_t big_count, int backend,
                           const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc,
                           double *mean_in, double *mean_out);
/* `sseq_de_from_sums_with_cancellation` (diff_exp.rs:208-300) on the device: scanrs_sseq_de_from_sums with the exact test's
 * backend (Cell Ranger's batched shared-control path passes Ratio, diff_exp.rs:172-175); scanrs_sseq_de_from_sums is this call
 * with LogSpace. Any other value of `backend` returns SCANRS_ERR_ARGUMENT. */
int scanrs_sseq_de_from_sums_backend(uint64_t n_genes, uint32_t n_tests, const uint64_t *sums_a, const uint64_t *sums_b, const double *sf_a,
                                     const double *sf_b, const double *gene_means, const double *gene_phi, const uint8_t *use_genes,
                                     uint64_t big_count, int backend, const scanrs_snoop *snoop, double *p, double *p_adj, double *log2fc,
                                     double *mean_in, double *mean_out);
/* Batched pairwise DE with per-pair parameters: the shape of merge_clusters.rs' candidates and of the shared-control batched path that
 * the doc comment of `sseq_params_from_moments` describes (diff_exp.rs:361-376: n_cells is "the cell count m = na + nb",
 * sum_size_factors "Σ(1/size_factor) over the test cells"). With A = the cells labelled pair_a[j] and B = those labelled pair_b[j],
 * test j is `compute_sseq_params(mat, zeta_quintile, Some(sorted A ∪ B), None)` (diff_exp.rs:458-490) followed by
 * `sseq_differential_expression_with_cancellation_backend(mat, A, B, params, big_count, backend)` (diff_exp.rs:125-161). All pairs
 * share two passes over the nonzeros (per-cell totals, then one grouped pass; from a gene-major copy one grouped pass per 1536
 * groups), and every pair's parameters are combined on the device from its two groups' integer sums: with u_c the total of cell c
 * and m_S the interpolated median total of the union, sf_c = u_c / m_S, Σ x/sf_c = m_S Σ x/u_c and Σ (x/sf_c)² = m_S² Σ (x/u_c)².
 * A pair's result depends on its own two groups only: not on the other pairs, the storage flag, or the copy that was walked.
 * Against the two reference calls the moments differ by the rounding of the sums (means to 1e-12, p-values to 1e-9 relative).
 * Labels as in scanrs_sseq_de (-1 .. n_groups - 1, n_groups <= 8192); outputs genes x n_pairs row-major. SCANRS_ERR_ARGUMENT: a
 * group index >= n_groups, pair_a[j] == pair_b[j], a pair whose union has no cell, n_pairs = 0, a bad backend, a sharded handle. A
 * pair with exactly one empty side is valid: that side's size factor is 0 and every p is 1, as in the reference. A pair whose
 * union has a median total of 0 (no finite size factor) runs the two reference calls themselves in the same call (`literal`).
 * So does a pair whose union holds a cell total u so large that a count of 1 in that cell would lose its bits under the call's one
 * quantum (terms x/u_c <= 1 under 2^(ilogb(cells) - 123): literal when (1/u)² keeps fewer than 33 bits, u above 2^35 at 2^20 cells):
 * scanrs_sseq_params gives every gene a quantum of its own there, and the moments of every pair keep the bounds stated with it.
 * Checkpoints of `snoop`: 0.0, 0.1 (totals and pair headers), 0.6 (grouped pass and parameters), 0.75, 0.9, 0.95, 1.0.
 * Counters (scanrs_mat_get_counter): "de_pairs_passes" = passes over the nonzeros in the last call (2, or 1 + the tiles of groups of a
 * gene-major copy, plus 4 per literal pair, 5 where that pair's scanrs_sseq_params walks the nonzeros once more for a quantum per
 * gene); "de_pairs_literal" = pairs that took the literal route.
 * `params` (may be NULL) receives what each pair was tested with. */
typedef struct {            /* every pointer may be NULL; arrays genes x n_pairs row-major, or n_pairs */
    double *gene_means, *gene_variances, *gene_moment_phi, *gene_phi;
    uint8_t *use_genes;
    double *zeta_hat, *delta, *sf_a, *sf_b, *median_total, *sum_size_factors;
    uint64_t *n_cells_a, *n_cells_b;
    uint8_t *literal;       /* 1: the pair took the literal route (median total 0, or a cell total beyond the shared quantum) */
} scanrs_sseq_pair_params;
int scanrs_sseq_de_pairs(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, const uint32_t *pair_a, const uint32_t *pair_b,
                         uint32_t n_pairs, double zeta_quintile, uint64_t big_count, int backend, const scanrs_snoop *snoop,
                         uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc, double *mean_in,
                         double *mean_out, scanrs_sseq_pair_params *params /* may be NULL */);
/* scanrs_sseq_de_pairs over a sharded matrix. scanrs_sseq_de_pairs_sharded is COLLECTIVE: every rank of the handle's
 * communicator (or host hook) calls it with the same arguments, which are those of scanrs_sseq_de_pairs. The CELLS must be the sharded
 * dimension (a handle sharded over the genes returns SCANRS_ERR_ARGUMENT), `labels` spans the WHOLE matrix (outer_global entries; each
 * rank uploads only its own slice), and every rank receives the same complete outputs. All argument checks run before the first
 * exchange and depend on the global arguments only. Every output, the per-pair parameters included, equals scanrs_sseq_de_pairs on
 * one unsharded handle of the whole matrix bit for bit, for any number of shards and any transport: only u64 sums cross the shards
 * (dtype 1 of scanrs_allreduce_fn) - the per-cell totals, the grouped accumulators (Σ x as it is, the two 128-bit moments as two
 * 32-bit halves of the low word plus the high word, in tiles of 2^20 (group, gene) entries through a fixed scratch of 56 MiB) and
 * the bit patterns of the p-values, whose tests are split over the ranks by gene as in scanrs_sseq_de. The group statistics, the pair
 * headers and the per-pair parameters run replicated on every rank from the reduced integers; a literal pair runs the sharded
 * scanrs_sseq_params + scanrs_sseq_de calls on every rank. Counters: "de_shard_allreduces" = the exchange steps of the last call
 * (2 + the accumulator tiles + 5 per literal pair, 6 where its moments take a quantum per gene: the genes' classes), "de_shard_tests" = the tests this rank launched. On an unsharded handle the call
 * is scanrs_sseq_de_pairs. scanrs_multi_sseq_de_pairs runs the collective call on every shard of a scanrs_multi from one process
 * (transposed != 0: the matrix was created cells x genes); shard 0 writes the caller's arrays and reports progress. */
int scanrs_sseq_de_pairs_sharded(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, const uint32_t *pair_a, const uint32_t *pair_b,
                                 uint32_t n_pairs, double zeta_quintile, uint64_t big_count, int backend, const scanrs_snoop *snoop,
                                 uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc, double *mean_in,
                                 double *mean_out, scanrs_sseq_pair_params *params /* may be NULL */);
int scanrs_multi_sseq_de_pairs(scanrs_multi *mm, int transposed, const int16_t *labels, uint32_t n_groups, const uint32_t *pair_a,
                               const uint32_t *pair_b, uint32_t n_pairs, double zeta_quintile, uint64_t big_count, int backend,
                               const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc,
                               double *mean_in, double *mean_out, scanrs_sseq_pair_params *params /* may be NULL */);
/* percentile_of_sorted(.., 50) (stat.rs:140-162) of the union of two ascending lists; host only */
int scanrs_host_union_median(const double *a, uint64_t n_a, const double *b, uint64_t n_b, double *out);
/* the shared math on the host (no device needed; the kernels run the same special functions): `nb_exact_test`
 * (dist.rs:74-118), `nb_asymptotic_test` (:226-257), `log_prob_all` (:259-310, n + 1 values: the terms scanrs_host_nb_exact_test
 * sums), `adjusted_pvalue_bh` (:22-50, out[i] belongs to p[i]), and the regularised incomplete beta function and its
 * inverse in p */
int scanrs_host_nb_exact_test(uint64_t x_a, uint64_t x_b, double sf_a, double sf_b, double mu, double phi, double *p);
int scanrs_host_nb_asymptotic_test(uint64_t x_a, uint64_t x_b, double sf_a, double sf_b, double mu, double phi, double *p);
/* `nb_exact_test_ratio` (dist.rs:155-215), host only, line for line: the three guards (exactly 1.0), the scan for the anchor, the
 * two sweeps, the serial sums, and the fallback to scanrs_host_nb_exact_test when the observed term is 0 or not finite. One line is
 * added: with sa_r == sb_r the mirror term n - x_a is extreme whatever its rounding (see scanrs_sseq_de_backend). */
int scanrs_host_nb_exact_test_ratio(uint64_t x_a, uint64_t x_b, double sf_a, double sf_b, double mu, double phi, double *p);
/* `nb_exact_ratio_step` (dist.rs:124-126), host only: T(k+1)/T(k) = (sa_r + k)(n - k) / ((k + 1)(sb_r + n - k - 1)) */
int scanrs_host_nb_exact_ratio_step(double k, double n, double sa_r, double sb_r, double *out);
int scanrs_host_nb_log_prob_all(uint64_t n, double sf_a, double sf_b, double mu, double r, double *out);
int scanrs_host_adjusted_pvalue_bh(const double *p, uint64_t n, double *out);
int scanrs_host_betainc(double a, double b, double x, double *out);
int scanrs_host_betaincinv(double a, double b, double p, double *out);

/* ---- merge_clusters (scan-rs/src/merge_clusters.rs, linkage.rs, stats.rs) ---------------------------------------------------
 * Labels are one int16 per cell with values 0 .. K-1, every value present, K <= 8192; anything else returns SCANRS_ERR_ARGUMENT
 * naming the first bad cell or the first missing label (the reference reads a leaf index as a label, which only means something
 * for contiguous labels). Scores are n x d f64, row-major with leading dimension ld >= d (elements); a NaN among them returns
 * SCANRS_ERR_ARGUMENT (the reference panics in n64). */

/* `pdist` (linkage.rs:14-26): x m x d row-major; out m (m - 1) / 2 Euclidean distances, pairs (i, j > i) in row order, each
 * summed over the dimensions in order then sqrt. Host only. */
int scanrs_host_pdist(const double *x, uint64_t m, uint32_t d, double *out);
/* `linkage(x, &Complete)` (linkage.rs:43-47, nn_chain :72-158, sort_by_column, relabel :160-216): z is (m - 1) x 4 f64 row-major in
 * the reference's layout [a, b, distance, size], rows by (distance, row). m >= 1; distances that are NaN are refused. Host only. */
int scanrs_host_linkage_complete(const double *x, uint64_t m, uint32_t d, double *z);
/* `relabel_by_size` (merge_clusters.rs:43-56): labels ordered by count, largest first, equal counts in ascending label order
 * (any int16 values). Host only. */
int scanrs_host_relabel_by_size(const int16_t *labels, uint64_t n, int16_t *out);
/* `medioids` (merge_clusters.rs:20-40): centers[i * d + j] is the median (`median_mut`, stats.rs:13-39: the middle of the sorted
 * list, the mean of the two middle values for an even count) of column j over the cells labelled i; labels 0 .. k-1, each present.
 * Exact radix select on the device (cluster.hip); ±0.0 may stand for each other. pca is a host array of n rows of ld elements. */
int scanrs_cluster_medoids(const double *pca, uint64_t n, uint32_t ld, uint32_t d, const int16_t *labels, uint32_t k, double *centers);
/* the same on scores already in device memory, e.g. scanrs_pca_result_device's *d_v / *ld_v; centers is a host array */
int scanrs_cluster_medoids_device(const double *d_pca, uint64_t n, uint32_t ld, uint32_t d, const int16_t *labels, uint32_t k, double *centers);

/* What scanrs_merge_clusters evaluated. The caller sets capacity and the four arrays (NULL when capacity is 0); entry i is the i-th
 * candidate in the reference's evaluation order: the two leaves (labels of that round, leaf0 < leaf1), the number of genes with
 * adjusted p < 0.05, and the smallest adjusted p (NaN values skipped; NaN when there is none). Entries past capacity are counted,
 * not stored. */
typedef struct {
    uint64_t capacity;
    int16_t *leaf0, *leaf1;
    uint64_t *n_de;
    double *min_p_adj;
    uint64_t n_candidates, n_rounds, n_merges; /* out: candidates evaluated, rounds of the loop (the last merges nothing), merges */
    uint64_t n_passes;                         /* out: passes over the nonzeros */
} scanrs_merge_trace;

/* `merge_clusters(fbm, pca, labels)` (merge_clusters.rs:59-138): merge, one pair per round, clusters that are adjacent under complete
 * linkage of their medoids and have no gene with BH-adjusted p < 0.05 between them; labels_out gets `relabel_by_size` of the result.
 * Rows of the handle are genes, columns are the n cells; DE reads the stored u32 counts and ignores map and offset (as scanrs_sseq_*
 * does); sharded handles are refused. pca (n x d, leading dimension ld) is a host array, or device memory when pca_is_device != 0
 * (PcaResultDevice.d_v / ld_v). n = 0 gives an empty result; a set cancel flag of `snoop` is read before every candidate
 * (SCANRS_ERR_CANCELLED; no progress is reported, as in the reference). trace may be NULL.
 * Handle option "merge_fused" (default 1): the per-cell totals, then ONE pass over the nonzeros that gathers per (gene, cluster)
 * Σ x, Σ x/u_c and Σ (x/u_c)² (u_c the cell's total; 128-bit fixed point) makes each candidate's params and sums an O(genes)
 * combination (a union whose median total is 0, or which holds a cell total beyond the shared quantum as in scanrs_sseq_de_pairs,
 * takes the literal route); 0: every candidate runs compute_sseq_params on the union
 * and the pairwise DE on the device, call for call as the reference (the A/B baseline). */
int scanrs_merge_clusters(scanrs_mat *m, const double *pca, int pca_is_device, uint32_t ld, uint32_t d, const int16_t *labels,
                          int16_t *labels_out, const scanrs_snoop *snoop, scanrs_merge_trace *trace);
/* merge_clusters and the medoids over a sharded matrix. scanrs_merge_clusters_sharded and
 * scanrs_cluster_medoids_sharded are COLLECTIVE: every rank of the handle's communicator (or host hook) calls them with the same
 * arguments, those of scanrs_merge_clusters and of scanrs_cluster_medoids (the handle of the latter only carries the transport and the
 * rank's range of cells). The CELLS must be the sharded dimension; `labels` spans the WHOLE matrix, and so does a host `pca`
 * (outer_global x ld, pca_is_device = 0), of which each rank uploads only its own rows; with pca_is_device != 0 the pointer holds the
 * rank's OWN cells only (local columns x ld, e.g. *d_v of scanrs_pca_result_device). labels_out, the trace and the centers are
 * complete and the same on every rank, and equal the unsharded call's bit for bit: only u64 sums cross the shards (dtype 1). A
 * median is selected exactly over the ranks: each of the 8 radix rounds adds the local keys that match the current prefix into
 * 256-bin integer histograms per (cluster, column, wanted rank), all-reduces the table (at most 4096 (cluster, column) pairs = 16 MiB
 * at a time) and picks the bucket on every rank; the first cell holding a NaN is the minimum over one slot per rank. The fused route
 * gathers the totals and reduces the grouped accumulators as scanrs_sseq_de_pairs_sharded does; the candidates then run replicated,
 * their tests split over the ranks by gene (one exchange per candidate); the literal route is the sharded scanrs_sseq_params +
 * scanrs_sseq_de. Every rank polls the cancel flag before the same candidates. Counters: "de_shard_allreduces" = the exchange steps
 * of the last call, "de_shard_tests" = the tests this rank launched. On an unsharded handle the calls are the plain ones.
 * scanrs_multi_merge_clusters / scanrs_multi_cluster_medoids run the collective calls on every shard of a scanrs_multi from one
 * process; pca is a host array over all cells. */
int scanrs_merge_clusters_sharded(scanrs_mat *m, const double *pca, int pca_is_device, uint32_t ld, uint32_t d, const int16_t *labels,
                                  int16_t *labels_out, const scanrs_snoop *snoop, scanrs_merge_trace *trace);
int scanrs_cluster_medoids_sharded(scanrs_mat *m, const double *pca, int pca_is_device, uint32_t ld, uint32_t d, const int16_t *labels,
                                   uint32_t k, double *centers);
int scanrs_multi_merge_clusters(scanrs_multi *mm, int transposed, const double *pca, uint32_t ld, uint32_t d, const int16_t *labels,
                                int16_t *labels_out, const scanrs_snoop *snoop, scanrs_merge_trace *trace);
int scanrs_multi_cluster_medoids(scanrs_multi *mm, int transposed, const double *pca, uint32_t ld, uint32_t d, const int16_t *labels,
                                 uint32_t k, double *centers);

/* ---- hclust: hierarchical clustering with leaf ordering (hclust/src/lib.rs) -------------------------------------------
 * HierarchicalCluster::new (hclust/src/lib.rs:132-148), leaves (:150-206), merge_clusters_below_distance_threshold (:210-227),
 * fcluster (:231-239), relabel_vector (:122-125). The metric is Euclidean (the reference's only one, :19-23): each squared distance
 * is the sum over the dimensions in order of (b_k - a_k)^2, multiply and add rounded separately, then the square root. The
 * dendrogram is kodama::linkage's: n - 1 steps sorted by dissimilarity (a stable sort of the merges in the order the chain found
 * them), the cluster made by sorted step i is named n + i, cluster1 < cluster2, size counts observations.
 * scanrs_hclust_create: x is a HOST array of rows x cols f64, row-major with leading dimension ld >= cols (elements); direction
 * says whether its rows or its columns are the observations. scanrs_hclust_create_device: the same on an array in device memory,
 * e.g. *d_u / *ld_u or *d_v / *ld_v of scanrs_pca_result_device. The distance pass and the nearest-neighbour chain run on the device
 * against a full symmetric n x n f64 matrix (n^2 * 8 bytes, both halves kept current); when that does not fit beside what the
 * library holds, SCANRS_ERR_DEVICE names n and the bytes. Fewer than two observations: SCANRS_ERR_SHAPE, "Need at least two elements
 * to do hierarchical clustering" (:134). A NaN or an infinity in x: SCANRS_ERR_ARGUMENT naming the first such element in row-major
 * order (as scanrs_merge_clusters refuses one). snoop may be NULL: a cancel flag that is already set returns SCANRS_ERR_CANCELLED
 * before anything is queued; afterwards the flag is read, and progress = merges / (n - 1) reported, between batches of chain steps.
 * Finite coordinates whose distance is not finite (squared differences overflow beyond about 1.3e154) return SCANRS_ERR_ARGUMENT
 * naming the first such pair of observations, after the distance pass and before any chain step. A Lance-Williams update whose
 * result is not finite (Ward on squared distances near the top of the f64 range) returns SCANRS_ERR_NUMERICAL: the update flags it
 * on the device and every later step returns at once, so no value that is not finite is ever scanned. On any failure *out is NULL
 * and what the call allocated on the device has been released. A chain that has not finished within 3 n steps returns
 * SCANRS_ERR_NUMERICAL as well (a chain of finite dissimilarities ends within 3 (n - 1)). Results are bit-reproducible (no floating-point atomics) and equal scanrs_host_hclust_linkage's.
 * NOT provided: Centroid and Median linkage. They are not reducible: the nearest-neighbour chain does not compute them, and kodama
 * runs a different algorithm for them. They return SCANRS_ERR_ARGUMENT naming the method. Also not provided: other metrics, optimal
 * leaf ordering, condensed-matrix input, a sharded form.
 * scanrs_hclust_from_steps (host only): a handle around a given dendrogram of n observations, n - 1 entries per array. Refused with
 * SCANRS_ERR_ARGUMENT unless every step's clusters were made by earlier steps (c < n + i), no cluster is merged twice, size[i] is the
 * sum of its clusters' sizes, and the dissimilarities are sorted and not NaN.
 * scanrs_hclust_steps fills n - 1 entries of each array that is not NULL. scanrs_hclust_leaves fills the n observations left to right
 * under SimpleOrdering (:74-116): NAIVE keeps the smaller cluster name on the left (:150-161), MODULAR_SMALLEST the side whose
 * smallest dissimilarity is <= the other's (:176-193). scanrs_hclust_merge_below unions every step with dissimilarity < threshold
 * (strictly) and labels the observations 1, 2, .. in order of first appearance. scanrs_hclust_fcluster: all ones for num_clusters
 * <= 1, otherwise merge_below(steps[n saturating_sub num_clusters].dissimilarity), so num_clusters >= n leaves every observation
 * alone and tied heights may give more clusters than asked for.
 * scanrs_hclust_info fills up to 7 values: [0] chain steps taken, [1] kernel launches issued, [2] batches of steps the host waited
 * for, [3] bytes of the distance matrix, [4] / [5] MICROSECONDS of the distance pass / of the chain between HIP events, [6] merges
 * made (n - 1). A handle from scanrs_hclust_from_steps reports zeros but [6].
 * scanrs_host_hclust_linkage (host only; tests and small inputs, n <= 20000): the same chain in plain C++ on n x d compact
 * observations, with the same tie rule, update formulas (csrc/hclust_lw.hpp) and summation order; the device result equals it bit
 * for bit. scanrs_debug_hclust_pdist: the device distance pass alone on x (n x d, leading dimension ld), squared or not, as a
 * condensed array in scanrs_host_pdist's order (n <= 8192). */
typedef struct scanrs_hclust scanrs_hclust;
enum { /* kodama::Method's order */
    SCANRS_LINKAGE_SINGLE = 0,
    SCANRS_LINKAGE_COMPLETE = 1,
    SCANRS_LINKAGE_AVERAGE = 2,
    SCANRS_LINKAGE_WEIGHTED = 3,
    SCANRS_LINKAGE_WARD = 4,
    SCANRS_LINKAGE_CENTROID = 5, /* not provided */
    SCANRS_LINKAGE_MEDIAN = 6    /* not provided */
};
enum { SCANRS_CLUSTER_ROWS = 0, SCANRS_CLUSTER_COLUMNS = 1 };       /* ClusterDirection (:30-35) */
enum { SCANRS_LEAF_NAIVE = 0, SCANRS_LEAF_MODULAR_SMALLEST = 1 }; /* LeafOrdering (:53-59) */
int scanrs_hclust_create(const double *x, uint64_t rows, uint64_t cols, uint64_t ld, int direction, int method, const scanrs_snoop *snoop,
                         scanrs_hclust **out);
int scanrs_hclust_create_device(const double *d_x, uint64_t rows, uint64_t cols, uint64_t ld, int direction, int method,
                                const scanrs_snoop *snoop, scanrs_hclust **out);
int scanrs_hclust_from_steps(uint64_t n, const uint32_t *c1, const uint32_t *c2, const double *diss, const uint32_t *size, scanrs_hclust **out);
void scanrs_hclust_free(scanrs_hclust *h);
int scanrs_hclust_n(const scanrs_hclust *h, uint64_t *n);
int scanrs_hclust_steps(const scanrs_hclust *h, uint32_t *c1, uint32_t *c2, double *diss, uint32_t *size);
int scanrs_hclust_leaves(const scanrs_hclust *h, int ordering, uint32_t *out);
int scanrs_hclust_merge_below(const scanrs_hclust *h, double threshold, uint32_t *labels);
int scanrs_hclust_fcluster(const scanrs_hclust *h, uint64_t num_clusters, uint32_t *labels);
int scanrs_hclust_info(const scanrs_hclust *h, uint64_t *out, uint32_t n_out);
int scanrs_host_hclust_linkage(const double *x, uint64_t n, uint32_t d, int method, uint32_t *c1, uint32_t *c2, double *diss, uint32_t *size);
int scanrs_debug_hclust_pdist(const double *x, uint64_t n, uint32_t d, uint64_t ld, int squared, double *out_condensed);

/* ---- knn over sharded and multi-GPU score matrices ----------------------------------------------------------------
 * knn(v, k) / find_nn (nn.rs:38-83) where the scores stay sharded: every rank owns the queries of its own cells, the point set
 * passes by in global blocks of "knn_block_rows" rows (each block reaches every rank through ONE u64 all-reduce of the rows' bit
 * patterns into a zeroed buffer; only dtype 1 crosses the shards), every block is searched with the kernels of scanrs_knn (the
 * filter where its conditions hold for the rank's queries and the block, seeded with what the query already holds) and merged into
 * the query's running list by (squared distance, global index). The answer is the k smallest pairs under that total order with the
 * same fma chain as scanrs_knn, so it EQUALS scanrs_knn of the whole point set bit for bit, whatever the cut; the self exclusion
 * compares global rows.
 * scanrs_knn_sharded (nn.rs:38-83): COLLECTIVE, every rank calls it with the same d and k. The handle carries the transport and the
 * rank's range of cells only (the columns of the view must be the sharded dimension). points: a host array over all outer_global
 * cells (leading dimension ld; each rank uploads its own rows), or with points_is_device != 0 the rank's own rows in device memory,
 * e.g. *d_v / *ld_v of scanrs_pca_result_device. out: host, n_local x k GLOBAL indices, nearest first, padded with UINT32_MAX when
 * fewer than k other points exist globally; sq_dist (may be null): n_local x k squared distances, +inf in padded slots. Limits of
 * scanrs_knn: k <= 128, d <= 128, n <= 2^32 - 2. A coordinate that is not finite is refused with SCANRS_ERR_ARGUMENT on every rank,
 * naming the first such global row (with a NaN the order is not total); ranks that disagree on n, d or k get SCANRS_ERR_ARGUMENT
 * from the first exchange, which carries four integers per rank. On an unsharded handle the call is scanrs_knn / scanrs_knn_device
 * on the given points. Counters (scanrs_mat_get_counter), reset by every call, 0 from an unsharded handle: "knn_blocks" = the blocks
 * searched, "knn_allreduces" = the exchange steps (blocks + 1). scanrs_debug_knn_last_stats describes the last block searched.
 * scanrs_multi_knn (nn.rs:38-83) runs the collective call on every shard of a scanrs_multi from one process; out / sq_dist cover all
 * cells in global order. points: a host array over all cells, or NULL: every shard searches the factor along the sharded dimension
 * that its last scanrs_multi_pca_bk / _rand left on its device (V of a genes x cells CSC matrix; ld and d are ignored, d is that
 * call's k). SCANRS_ERR_ARGUMENT when no PCA has run, or where that factor is not kept per shard (it then has other than the
 * shard's own rows on the device: pass the scores as a host array).
 * scanrs_host_knn_merge (nn.rs:38-83; host only): the merge rule itself. Two lists of k (squared distance, index) entries, ascending by
 * (distance, index), padded with (+inf, UINT32_MAX), sharing no index, give the first k of their union in the same form. k <= 128. */
int scanrs_knn_sharded(scanrs_mat *m, const double *points, int points_is_device, uint32_t ld, uint32_t d, uint32_t k, uint32_t *out,
                       double *sq_dist);
int scanrs_multi_knn(scanrs_multi *mm, const double *points, uint32_t ld, uint32_t d, uint32_t k, uint32_t *out, double *sq_dist);
int scanrs_host_knn_merge(uint32_t k, const double *da, const uint32_t *ia, const double *db, const uint32_t *ib, double *dout,
                          uint32_t *iout);

/* ---- nearest_neighbors under Euclidean, Pearson and cosine distance (umap-rs/src/knn.rs, dist.rs) -------------------
 * umap_rs::knn::nearest_neighbors(data, k, distance_type, num_threads) -> (knn_indices, knn_distances): the pair every embedding
 * stage downstream starts from (umap.rs:89). data: n x d row-major f64. `enum DistanceType` (dist.rs:12-35): */
enum { SCANRS_DIST_EUCLIDEAN = 0, SCANRS_DIST_PEARSON = 1, SCANRS_DIST_COSINE = 2 };
/* The value of a pair under pearson and cosine is the reference's own formula, every operation a separate IEEE f64 operation in
 * coordinate order, nothing fused (dist.rs:73-84, 106-124): cosine folds s_xx, s_yy, s_xy over x and y; pearson first subtracts
 * mu = fold(acc + x_j) / d from each row; then D = 0 if s_xx == 0 && s_yy == 0, else 1 if s_xy == 0, else
 * max(1 - s_xy / sqrt(s_xx s_yy), 0) with f64::max (a NaN operand loses: 0). The search orders by key = sqrt(D) and returns
 * key * key (metric / metric2dist, dist.rs:19-34) - generally not the bits of D. Ties, including the ones sqrt creates, come in
 * ascending index order, the rule of scanrs_knn (the vp-tree's order among equal keys is a property of that crate). The answer is
 * reproducible bit for bit: the device search equals scanrs_host_nearest_neighbors in indices and distance bit patterns.
 * DEVIATION, euclidean only: the reference calls simd_euclidean::Vectorized::distance (dist.rs:86-89), whose summation order is
 * not in the reference tree. This kind is the library's existing search: ordered by (squared distance as scanrs_knn forms it - one
 * fma chain in coordinate order -, index), the returned distance the square root of that: a few ulp from the reference's value.
 * A row is never its own neighbour (knn.rs:155). k_eff = min(k, n - 1) (knn.rs:124-127): the C entry points write n x k and pad
 * columns k_eff .. k-1 with UINT32_MAX / +inf (the reference's initial fill, knn.rs:139-140; the padding rule of scanrs_knn).
 * Limits of scanrs_knn: k <= 128, d <= 128, n <= 2^32 - 2. A coordinate that is not finite is refused with SCANRS_ERR_ARGUMENT,
 * naming the first such row (with a NaN the order is not total). n < 2 or k == 0: nothing beyond padding is written, success.
 * Routes (pearson, cosine): an exhaustive kernel for every shape, and - from "knn_filter_min_points" points on, d <= 58, k <= 64,
 * at least 256 rows, no degenerate row (s_xx == 0), every s_xx inside [2^-400, 2^400] - the bf16-MFMA filter of scanrs_knn on the
 * standardised rows with a threshold converted rigorously from the query's k-th key, every pair that passes ranked by the
 * reference formula. Options "knn_exhaustive", "knn_filter_min_points", "knn_ratio", "knn_stats" apply;
 * scanrs_debug_knn_last_stats tells which route the last call took.
 * NOT provided: the layout after the neighbour lists and their graph (the graph: scanrs_fuzzy_simplicial_set below).
 * scanrs_nearest_neighbors (knn.rs:112-166): data, indices, distances are host arrays.
 * scanrs_nearest_neighbors_query (knn.rs:112-166): a query set of its own. queries n_q x d and points n_p x d are host arrays;
 * indices / distances: n_q x k, the indices are rows of `points`. include_self == 0 drops the point whose index equals the query's
 * row number (the rule of scanrs_find_nn, meaningful when the two sets coincide); a row with fewer than k admissible points is
 * padded with UINT32_MAX / +inf. Limits, routes and refusals of scanrs_nearest_neighbors (the filter asks for at least 256 queries
 * and "knn_filter_min_points" points, and for the s_xx window on both sides); a row that is not finite is named with its set
 * ("queries" / "points"). With queries == points and include_self == 0 the answer is scanrs_nearest_neighbors' in every bit.
 * scanrs_nearest_neighbors_query_device (knn.rs:112-166): both sets in device memory, leading dimensions ld_q, ld_p >= d.
 * scanrs_host_nearest_neighbors_query (knn.rs:112-166; host only): the same answer by exhaustive search on the host (any k).
 * scanrs_nearest_neighbors_sharded (knn.rs:112-166): COLLECTIVE, over a sharded point set, with the argument conventions of
 * scanrs_knn_sharded: points is a host array over all outer_global cells, or with points_is_device != 0 the rank's own rows in
 * device memory; indices / distances: host, n_local x k, GLOBAL indices. The result EQUALS scanrs_nearest_neighbors of the whole
 * point set in indices and distance bit patterns, for every cut, world size, block size and route; ties, including the ones sqrt
 * creates, go by ascending global index. The first exchange carries n, d, k, distance_type and (first bad global row + 1) per rank:
 * ranks that disagree get SCANRS_ERR_ARGUMENT, a coordinate that is not finite is refused on every rank, naming the global row.
 * Then blocks of "knn_block_rows" RAW rows pass through one u64 all-reduce each; every rank prepares the block's rows itself (the
 * same bits everywhere), searches it with the query's k-th key so far as a strict seed - through the filter where the shape
 * conditions hold for (local queries, block) and both sides lie in the s_xx window, exhaustively otherwise - and merges the block's
 * list into the query's running list by (key, global index). Euclidean: scanrs_knn_sharded, then the square root. On an unsharded
 * handle the call is scanrs_nearest_neighbors / _device on the given points. Counters (scanrs_mat_get_counter), reset by every call:
 * "knn_blocks" and "knn_allreduces" as for scanrs_knn_sharded, and "knn_blocks_filtered" = the blocks this rank searched through
 * the filter (pearson and cosine; the route never changes a bit of the answer, so the ranks need not agree on it).
 * scanrs_multi_nearest_neighbors (knn.rs:112-166) runs the collective call on every shard of a scanrs_multi from one process, as
 * scanrs_multi_knn does: indices / distances cover all cells in global order; points == NULL searches the factor the last
 * scanrs_multi_pca_bk / _rand left on the devices, with the same refusals when there is none.
 * scanrs_nearest_neighbors_device (knn.rs:112-166): the points are already in device memory (n x d, leading dimension ld >= d
 * elements; what lies behind column d is never read), e.g. *d_v / *ld_v of scanrs_pca_result_device; indices / distances host.
 * scanrs_host_nearest_neighbors (knn.rs:112-166; host only): the same answer by exhaustive search on the host (any k).
 * scanrs_host_distance (dist.rs:19-34, 73-124; host only): one pair: *key = the rank key (sqrt(D); euclidean: the distance),
 * *dist = metric2dist(key) (key * key; euclidean: key).
 * scanrs_host_metric_rows (dist.rs:73-76, 106-115; host only): what the search forms once per row, exactly as the device forms
 * it: c (n x d) the centred row (pearson) or the row (cosine), s (n) its s_xx, z (n x d, may be null) = c / sqrt(s_xx), the
 * standardised row only the filter reads (all zero for a degenerate row). distance_type 1 or 2.
 * scanrs_debug_nearest_neighbors_params (host only; the filtered route's constants): the filter's threshold in the
 * space of the standardised rows is tau = 2 key_k^2 (1 + *delta) + *e, of which *chain is the allowance for the filter's own
 * fma chain; [*sxx_min, *sxx_max] is the magnitude window of s_xx outside which the filter declines. */
int scanrs_nearest_neighbors(const double *data, uint64_t n, uint32_t d, uint32_t k, int distance_type, uint32_t *indices,
                             double *distances);
int scanrs_nearest_neighbors_device(const double *d_data, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int distance_type,
                                    uint32_t *indices, double *distances);
int scanrs_host_nearest_neighbors(const double *data, uint64_t n, uint32_t d, uint32_t k, int distance_type, uint32_t *indices,
                                  double *distances);
int scanrs_nearest_neighbors_query(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k,
                                   int distance_type, int include_self, uint32_t *indices, double *distances);
int scanrs_nearest_neighbors_query_device(const double *d_queries, uint64_t n_q, uint32_t ld_q, const double *d_points, uint64_t n_p,
                                          uint32_t ld_p, uint32_t d, uint32_t k, int distance_type, int include_self, uint32_t *indices,
                                          double *distances);
int scanrs_host_nearest_neighbors_query(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k,
                                        int distance_type, int include_self, uint32_t *indices, double *distances);
int scanrs_nearest_neighbors_sharded(scanrs_mat *m, const double *points, int points_is_device, uint32_t ld, uint32_t d, uint32_t k,
                                     int distance_type, uint32_t *indices, double *distances);
int scanrs_multi_nearest_neighbors(scanrs_multi *mm, const double *points, uint32_t ld, uint32_t d, uint32_t k, int distance_type,
                                   uint32_t *indices, double *distances);
int scanrs_host_distance(int distance_type, const double *x, const double *y, uint32_t d, double *key, double *dist);
int scanrs_host_metric_rows(int distance_type, const double *data, uint64_t n, uint32_t d, double *c, double *s, double *z);
int scanrs_debug_nearest_neighbors_params(double *delta, double *e, double *chain, double *sxx_min, double *sxx_max);

/* ---- fuzzy_simplicial_set: the UMAP graph of the neighbour lists (umap-rs/src/fuzzy.rs, embedding.rs) ---------------
 * umap_rs::fuzzy::fuzzy_simplicial_set(knn_indices, knn_distances, local_connectivity, set_operation_ratio, apply_fuzzy_combine,
 * n_iter, bandwidth) -> CsMat (fuzzy.rs:30-62, called at umap.rs:92-100), and the pruned edge list of
 * initialize_simplicial_set_embedding (embedding.rs:29-54) up to but NOT including its shuffle. The reference's formulas literally,
 * every operation a separate IEEE f64 operation:
 *  rho (fuzzy.rs:79-99) from the row's distances > 0 in column order (+inf counts); where the reference would index past their end
 *    (non_zero_dist[index] with index == len, or non_zero_dist[0] of an empty list with floor(local_connectivity) == 0) the call is
 *    refused, naming the first such row.
 *  sigma (smooth_knn_dist, fuzzy.rs:117-145): target = log2(k) * bandwidth with k the width of the lists; psum folds
 *    exp(-(max(max(v, -rho), 0) / mid)) - v, not v - rho, as the reference writes it -; at most n_iter bisection steps.
 *  The floor (fuzzy.rs:103-111): rows with rho > 0 by their own mean distance, the others by the global mean. DEVIATION: the
 *    reference's global mean is one sequential fold over all n * k distances; the library adds the rows' left folds in a fixed tree
 *    whose shape depends on n alone (at most 2 n k 2^-53 relative from the reference's sum; it reaches only sigma of rows whose rho
 *    is not > 0, and with local_connectivity >= 1 no graph value depends on it).
 *  Membership (fuzzy.rs:161-178): entries with index UINT32_MAX are skipped; the value is 0 where the column POSITION j equals the
 *    neighbour's index (`j == knn_indices[[i, j]]`, literally), 1 where d - rho <= 0 or sigma == 0, else exp(-((d - rho) / sigma));
 *    it is R[index, i]: row = the neighbour, column = i.
 *  Union (fuzzy.rs:52-58) at every position of the pattern of R and its transpose, a missing operand read as +0.0:
 *    (r + t - r t) ratio + (r t)(1 - ratio), five operations. Zeros are stored like any other value.
 *  exp is the library's own (scanrs_host_fuzzy_exp), within 1 ulp like the libm the reference calls, the same source on the host and
 *    on the device: the device result EQUALS scanrs_host_fuzzy_simplicial_set in every bit of every output.
 * DEVIATION: an index a row names twice is refused. sprs' TriMat would add the two entries, but no neighbour list of the reference
 * names a row twice.
 * Refused with SCANRS_ERR_ARGUMENT: n == 0 or k == 0 (the reference asserts); k > 128; n > 2^32 - 2; local_connectivity not finite
 * or < 0; set_op_mix_ratio not finite; and per row, naming the first one: a NaN distance, an index that is neither < n nor
 * UINT32_MAX, the rho cases above, a repeated index. A refused or failed call leaves no handle and no device memory behind.
 * The sharded and multi-GPU forms are not provided. */
typedef struct scanrs_graph scanrs_graph;
typedef struct scanrs_fuzzy_params {
    double local_connectivity;   /* as in the reference (umap.rs: 1.0) */
    double set_op_mix_ratio;     /* as in the reference (umap.rs: 1.0) */
    int32_t apply_fuzzy_combine; /* 0: the graph is R itself (fuzzy.rs:48-50) */
    uint32_t n_iter;             /* 0 = the reference's 64 (fuzzy.rs:8) */
    double bandwidth;            /* 0.0 = the reference's 1.0 (fuzzy.rs:7) */
} scanrs_fuzzy_params;
/* scanrs_fuzzy_simplicial_set (fuzzy.rs:30-62): knn_indices (u32) / knn_distances (f64): host arrays, n x k, UINT32_MAX / +inf padding
 * accepted (what scanrs_nearest_neighbors writes). *graph: CSR resident on the device: u64 indptr (n + 1), u32 indices ascending
 * within a row, f64 values.
 * scanrs_fuzzy_simplicial_set_device (fuzzy.rs:30-62): the lists in device memory, both with leading dimension ld >= k.
 * scanrs_umap_graph (umap.rs:89-100): the search of scanrs_nearest_neighbors on host points (n x d), key -> distance, then the
 * graph, with nothing over the host link in between. The width of the lists is min(k, n - 1) (knn.rs:124-127), and that width is
 * the k of target. The result EQUALS scanrs_fuzzy_simplicial_set of scanrs_nearest_neighbors' output in every bit; the euclidean
 * kind inherits that search's stated deviation. Refusals of both.
 * scanrs_umap_graph_device (umap.rs:89-100): the points in device memory, leading dimension ld >= d.
 * scanrs_host_fuzzy_simplicial_set (fuzzy.rs:30-62; host only): the twin; its graph lives in host memory and answers the same
 * accessors (scanrs_graph_device refuses it).
 * scanrs_graph_info (fuzzy.rs:39): out[0] = n, out[1] = nnz, out[2] = the width of the lists, out[3] = 1 where the graph is resident
 * on the device; n_out values are written.
 * scanrs_graph_to_host (fuzzy.rs:47): indptr (n + 1), indices (nnz), values (nnz) into host arrays.
 * scanrs_graph_sigmas_rhos (fuzzy.rs:43): the pair smooth_knn_distances returns, n each.
 * scanrs_graph_device (fuzzy.rs:47): the device addresses of the three CSR arrays, valid until scanrs_graph_free.
 * scanrs_graph_free (fuzzy.rs:47): null is a no-op.
 * scanrs_graph_edge_count (embedding.rs:38-49): how many entries survive: graph_max = the maximum of the values folded from 0.0; a
 * value < graph_max / n_epochs becomes 0; values != 0.0 remain. n_epochs must be > 0. The graph is not modified.
 * scanrs_graph_edges (embedding.rs:38-53, 75-85): those entries in CSR order (rows ascending, columns ascending): tail = row,
 * head = column, weight, and epochs_per_sample = n_epochs / ((w / max_w) * n_epochs) where that product is > 0, else -1. Host
 * arrays of scanrs_graph_edge_count entries. The shuffle (embedding.rs:51) is not part of this.
 * scanrs_host_fuzzy_exp (fuzzy.rs:126, 171; host only): the library's exponential, element by element. exp(+-0) = 1, exp(-inf) = 0,
 * NaN -> NaN, gradual underflow.
 * scanrs_host_smooth_knn_dist (fuzzy.rs:117-145; host only): sigma of one row of k distances for a given rho; *iterations (may be
 * null) = how many times psum was formed. n_iter 0 = 64, bandwidth 0.0 = 1.0.
 * scanrs_host_membership_strengths (fuzzy.rs:148-181; host only): the COO triple (rows, cols, values; room for n * k each) and
 * *count of them. Indices are not checked (repeated ones included: the reference's own table has one). */
int scanrs_fuzzy_simplicial_set(const uint32_t *knn_indices, const double *knn_distances, uint64_t n, uint32_t k,
                                const scanrs_fuzzy_params *params, scanrs_graph **graph);
int scanrs_fuzzy_simplicial_set_device(const uint32_t *d_knn_indices, const double *d_knn_distances, uint64_t n, uint32_t ld, uint32_t k,
                                       const scanrs_fuzzy_params *params, scanrs_graph **graph);
int scanrs_umap_graph(const double *points, uint64_t n, uint32_t d, uint32_t k, int distance_type, const scanrs_fuzzy_params *params,
                      scanrs_graph **graph);
int scanrs_umap_graph_device(const double *d_points, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int distance_type,
                             const scanrs_fuzzy_params *params, scanrs_graph **graph);
int scanrs_host_fuzzy_simplicial_set(const uint32_t *knn_indices, const double *knn_distances, uint64_t n, uint32_t k,
                                     const scanrs_fuzzy_params *params, scanrs_graph **graph);
int scanrs_graph_info(const scanrs_graph *graph, uint64_t *out, uint32_t n_out);
int scanrs_graph_to_host(const scanrs_graph *graph, uint64_t *indptr, uint32_t *indices, double *values);
int scanrs_graph_sigmas_rhos(const scanrs_graph *graph, double *sigmas, double *rhos);
int scanrs_graph_device(const scanrs_graph *graph, const uint64_t **d_indptr, const uint32_t **d_indices, const double **d_values);
void scanrs_graph_free(scanrs_graph *graph);
int scanrs_graph_edge_count(const scanrs_graph *graph, double n_epochs, uint64_t *count);
int scanrs_graph_edges(const scanrs_graph *graph, double n_epochs, uint32_t *head, uint32_t *tail, double *weights,
                       double *epochs_per_sample);
int scanrs_host_fuzzy_exp(const double *x, uint64_t count, double *out);
int scanrs_host_smooth_knn_dist(const double *distances, uint32_t k, double rho, double bandwidth, uint32_t n_iter, double *sigma,
                                uint32_t *iterations);
int scanrs_host_membership_strengths(const uint32_t *knn_indices, const double *knn_distances, uint64_t n, uint32_t k, const double *sigmas,
                                     const double *rhos, uint32_t *rows, uint32_t *cols, double *values, uint64_t *count);

/* ---- the plan of the fixed-point column moments (option "col_moments"; host only, no device) -----------------------------------
 * The route adds, per slice, the terms f of the map as 64-bit integers rint(f 2^e1) (and rint(f^2 2^e2)): one quantum q = 2^-e for
 * the whole matrix, so every term is off by at most q/2 ABSOLUTE. The plan decides from global numbers whether that is good enough
 * for every slice, and chooses e1 / e2. Inputs: max_count, the largest stored count; the links of the map in order, kinds[i] = 1
 * (ScaleAxis) or 2 / 3 / 4 (ln, log2, log10 of 1 + x); for a ScaleAxis link on_summed_axis[i] != 0 when its factors belong to the
 * positions that are summed over, fmin_pos[i] its smallest factor > 0 and fmax[i] its largest factor (a link that holds a negative or
 * non-finite factor: pass such a value as fmax); n_outer = positions summed over, n_inner = slices, n_wg = workgroups the
 * positions are dealt over (min(compute units, ceil(n_outer / 64))), mode 1 = sums only, 2 = sums and sums of squares. The rule:
 *   - refused: a link of another kind, a ScaleAxis link on the other axis or with a negative / non-finite factor or with no positive
 *     factor, no logarithm in the chain, n_outer = 0, n_inner = 0 (a zero factor beside positive ones is fine: its terms are exactly 0);
 *   - x = the chain applied to max_count under every link's fmax (no term is larger), v_min = the chain applied to count 1 under every
 *     link's fmin_pos (no nonzero term is smaller), each widened by 1e-4 for the roundings of the bound itself;
 *   - e1 = the largest exponent with x 2^e1 <= 2^50 and ceil(n_outer / n_wg) x 2^e1 <= 2^62; e2 the same for x^2;
 *   - accepted when v_min 2^e1 >= 2^40 and (mode 2) v_min^2 2^e2 >= 2^33: a slice of n terms sums to at least n v_min and is off by at
 *     most n q/2, so its sum is right to 2^-41 = 4.6e-13 relative and its sum of squares to 2^-34 = 5.9e-11, which keeps sum and mean
 *     within 1e-12 relative and the variance within 1e-10 S2/m.
 * accept = 1 / 0; e1, e2 are meaningful when accepted. */
int scanrs_host_col_moments_plan(uint32_t max_count, uint32_t n_links, const int *kinds, const int *on_summed_axis, const double *fmin_pos,
                                 const double *fmax, uint64_t n_outer, uint64_t n_inner, uint32_t n_wg, int mode, int *accept, int *e1,
                                 int *e2);

/* ---- the route of a sparse product (host only, no device): csrc/spmm_route.hpp, the source launch_spmm_f64 decides by --------------
 * options: 18 values in this order - "spmm_path" (scanrs_mat_set_spmm_path), "panel_precision" (scanrs_mat_set_panel_precision), "tile_auto", "tile_k", "tile_s", "tile_t", "tile_b", "tile_ku",
 * "tile_dense", "tile_builder", "blocked_min_nnz", "slice_walk", "spmv_lds", "spmv_row_table", "spmm_order", "materialize",
 * "tile_wtab", "tile_fold", each checked like the option of its name ("blocked_min_nnz", default 2^22 and no key of
 * scanrs_mat_set_option: a whole number in [0, 2^63)) - a value an option would refuse returns SCANRS_ERR_ARGUMENT; n_outer, n_inner, nnz: the copy the product walks; l columns of a panel with leading dimension ldx; the map
 * as seen from that copy: kinds[i] = 1 ScaleAxis, 2 / 3 / 4 ln / log2 / log10 of 1 + x, 5 square, 6 / 7 the binomial deviance / Pearson
 * residuals, a_outer[i] != 0 when link i indexes its array by the outer position. flags stand for the two steps that need a device:
 * SCANRS_SPMM_TILES_AVAILABLE = a tile layout exists or was built (auto path: the size, the free memory and the overflow limit
 * allowed it), SCANRS_SPMM_NO_VALUES_ROOM = no memory for materialized map values. out[6]: the family (SCANRS_SPMM_*), the form and
 * the chunks as the counters "spmm_route" / "spmm_form" / "spmm_chunks" give them, the chunk width (tiles), 1 when the family
 * refuses odd leading dimensions, 1 when the product is a candidate for the tile route before the layout is asked for. */
#define SCANRS_SPMM_TILES_AVAILABLE 1u
#define SCANRS_SPMM_NO_VALUES_ROOM 2u
int scanrs_host_spmm_route(const double *options, uint64_t n_outer, uint64_t n_inner, uint64_t nnz, uint32_t l, uint32_t ldx,
                           uint32_t n_links, const int *kinds, const int *a_outer, uint32_t flags, uint64_t *out);

/* ---- the tables of options and counters (host only, no device): csrc/options.cpp, the source the setters and the getter decide by
 * scanrs_host_option_info: row `index` of the options of a handle (scope 0) or of the process (scope 1); SCANRS_ERR_ARGUMENT past
 * the end. name: the key; dflt: the default, in the key's own unit; lo, hi: the bounds (of a flag: 0 and 1; hi may be infinite);
 * flags: SCANRS_OPTION_OPEN_LO = lo itself is refused, SCANRS_OPTION_SETTABLE = a key of scanrs_mat_set_option /
 * scanrs_set_global_option (the three rows without it are read by the route decision and set elsewhere or never), and from bit
 * SCANRS_OPTION_ROUTE_SHIFT on the option's position + 1 in the `options` array of scanrs_host_spmm_route (0: not in it).
 * scanrs_host_option_parse: what the setter of that scope would store for `value` under the key `name` (bytes for the keys in KB,
 * 0 / 1 for a flag, the clamped number for a global option that clamps) - or the setter's refusal, SCANRS_ERR_ARGUMENT: an unknown
 * or unsettable key, a value that is not finite, outside the bounds or not whole where the key takes whole numbers. Nothing is stored.
 * scanrs_host_counter_name: key `index` of scanrs_mat_get_counter; SCANRS_ERR_ARGUMENT past the end. */
#define SCANRS_OPTION_OPEN_LO 1u
#define SCANRS_OPTION_SETTABLE 2u
#define SCANRS_OPTION_ROUTE_SHIFT 8
int scanrs_host_option_info(int scope, uint32_t index, const char **name, double *dflt, double *lo, double *hi, uint32_t *flags);
int scanrs_host_option_parse(int scope, const char *name, double value, double *stored);
int scanrs_host_counter_name(uint32_t index, const char **name);

/* ---- the projection plan of svd_bk (host only, no device): csrc/bk_plan.hpp, the source the solver decides by ---------------------
 * svd_bk forms its projection as T' = (op(A) K) C from the half-products of its iterations; a column of Q whose coefficient column
 * reaches the bound "reuse_cmax" is recomputed by a sparse product instead. colmax[n]: max |C| per column of Q, n = b * n_iter
 * (b the block width, even for the scheme to apply); coef_valid = 0 when a rank-deficient panel was completed on the host, which voids
 * the coefficients. out[7]: 1 when b is even, the older blocks' columns at or above reuse_cmax (before any raise), the branch of the
 * raise rule (as the counter "bk_limit_branch"), the number of direct columns, 1 when the whole last block is among them, 1 when the
 * projection is one n-wide product instead, the blocks projected beside the sparse passes. limit: the bound finally used;
 * cmax_dense: the largest entry of colmax among the columns that take the dense route (0 without one); direct[n]: the first out[3]
 * entries are the direct columns in the order the repair pass carries them (older blocks ascending, then the last block).
 * Refused (SCANRS_ERR_ARGUMENT): b = 0, n_iter = 0, n != b * n_iter, a negative or non-finite entry of colmax, reuse_cmax that is
 * not positive. */
int scanrs_host_bk_plan(const double *colmax, uint64_t n, uint32_t b, uint32_t n_iter, double reuse_cmax, int coef_valid, uint64_t *out,
                        double *limit, double *cmax_dense, uint32_t *direct);
/* Which sort the transposed copy of a matrix is built through (csrc/transpose_plan.hpp, the source copy_build.hip decides by), on the
 * host: n_outer x n_inner are the dimensions of the copy that is transposed, max_value its largest stored count (0: not known, the
 * count takes 32 bits). ib / ob / cb: the bits that hold 0 .. n_inner - 1, 0 .. n_outer - 1 and 0 .. max_value (at least 1 each);
 * route: 1 (one packed 64-bit key per nonzero) when ib + ob + cb <= 64, else 2 (a u32 key with a u64 value). The counter
 * "transpose_route" of a handle gives the route a build took. Refused (SCANRS_ERR_SHAPE): a dimension beyond 2^32 - 1. */
int scanrs_host_transpose_plan(uint64_t n_outer, uint64_t n_inner, uint32_t max_value, int *route, uint32_t *ib, uint32_t *ob, uint32_t *cb);

/* ---- 10x HDF5 ingestion (hdf5-io/src/matrix.rs, analysis.rs). Host-side; no device needed.
 * The files are parsed by the library's own reader (csrc/h5lite.cpp) — no libhdf5 dependency. Failures are
 * SCANRS_ERR_IO with the reason in scanrs_last_error(). ------------------------------------------------------------ */
typedef struct scanrs_h5_matrix scanrs_h5_matrix; /* GenericFeatureBarcodeMatrix / MatrixMetadata (scan-types/src/matrix.rs:8-15) */

/* `read_csc_matrix` (hdf5-io/src/matrix.rs:56-97): group "matrix" -> features x barcodes CSC, u64 indptr, u32 indices,
 * u32 values (stored values converted through f64 as the reference does, :247-257). Columns whose indices are not
 * ascending (some Cell Ranger 3 files) are sorted, the reference's `new_from_unsorted_csc` fallback (:71-79). */
int scanrs_h5_read_csc_matrix(const char *path, scanrs_h5_matrix **out);
/* `read_adaptive_csr_matrix` (:129-199): the same matrix feature-major (CSR) with features dropped when their
 * feature_type does not contain `retain_feature_like` (NULL: keep all) or their total count is below `shrink_row`
 * (< 0: None). The arrays are exactly what scanrs_mat_create(rows, cols, SCANRS_CSR, ...) takes. */
int scanrs_h5_read_adaptive_csr_matrix(const char *path, const char *retain_feature_like, int64_t shrink_row,
                                       scanrs_h5_matrix **out);
/* `read_matrix_metadata` (:17-54): barcodes, (filtered) feature ids / names / types and nnz; no matrix arrays. */
int scanrs_h5_read_matrix_metadata(const char *path, const char *retain_feature_like, scanrs_h5_matrix **out);
void scanrs_h5_matrix_free(scanrs_h5_matrix *m);

int scanrs_h5_matrix_shape(const scanrs_h5_matrix *m, uint64_t *rows, uint64_t *cols, uint64_t *nnz, int *storage);
/* borrowed pointers, valid until scanrs_h5_matrix_free; NULL for a metadata-only handle */
int scanrs_h5_matrix_arrays(const scanrs_h5_matrix *m, const uint64_t **indptr, const uint32_t **indices, const uint32_t **values);
/* what = 0 barcodes, 1 feature ids, 2 feature names, 3 feature types (per kept feature; the LabelClass of the reference
 * flattened, scan-types/src/label_class.rs:129-145), 4 name of the file */
int scanrs_h5_matrix_n_strings(const scanrs_h5_matrix *m, int what, uint64_t *n);
const char *scanrs_h5_matrix_string(const scanrs_h5_matrix *m, int what, uint64_t i);
/* indices (in the file's feature order) of the features that were filtered out — the BTreeSet the reference returns */
int scanrs_h5_matrix_removed(const scanrs_h5_matrix *m, const uint64_t **removed, uint64_t *n);

/* One call from a file to the device handle: `read_adaptive_csr_matrix` (or `load_mtx` when `path` does not end in
 * ".h5") followed by scanrs_mat_create on the CSR arrays. `meta` (optional) receives the host-side handle with the
 * barcodes / feature tables / removed set; free it with scanrs_h5_matrix_free. Needs a gfx950 device. */
int scanrs_mat_create_from_file(const char *path, const char *retain_feature_like, int64_t shrink_row, scanrs_mat **out,
                                scanrs_h5_matrix **meta);
/* scanrs_mat_create_from_file's multi-GPU form (cmd.rs:61-70): read_adaptive_csr_matrix for a path ending in ".h5"
 * (hdf5-io/src/matrix.rs:119-192), load_mtx otherwise (scan-rs/src/mtx.rs:10-51), then scanrs_multi_create_inner on the CSR arrays.
 * `meta` (optional) as in scanrs_mat_create_from_file. */
int scanrs_multi_create_from_file(const char *path, const char *retain_feature_like, int64_t shrink_row, uint32_t n_shards,
                                  const int *devices, scanrs_multi **out, scanrs_h5_matrix **meta);

/* `load_mtx` (scan-rs/src/mtx.rs:10-51): gzipped MatrixMarket coordinate file -> CSR arrays in the same handle type
 * (no string tables; scanrs_h5_matrix_arrays / _shape / _free apply). Comments '%', header "NROW NCOL NNZ", 1-based
 * "ROW COL VAL" triplets with u32 values, duplicates summed, indices ascending inside a row (TriMat::to_csr). */
int scanrs_mtx_read(const char *path, scanrs_h5_matrix **out);

/* `read_umi_counts_from_matrix` (:270-299): per-barcode sums of the stored values, read in blocks of 2000 columns */
int scanrs_h5_read_umi_counts(const char *path, uint32_t *out, uint64_t cap, uint64_t *n);

/* `get_clustering_keys` (analysis.rs:38-41): names under /clustering, NUL-separated into buf */
int scanrs_h5_get_clustering_keys(const char *path, char *buf, uint64_t cap, uint64_t *n_keys, uint64_t *bytes);
/* `get_clustering` (analysis.rs:5-20): i64 -> i16 / u16 by truncation, as the reference's `as` casts do */
int scanrs_h5_get_clustering(const char *path, const char *clustering_key, uint16_t *num_clusters, int16_t *clusters,
                             uint64_t cap, uint64_t *n);
/* `get_differential_expression` (analysis.rs:23-36): the rows x cols f64 table, row-major */
int scanrs_h5_get_differential_expression(const char *path, const char *clustering_key, double *out, uint64_t cap,
                                          uint64_t *rows, uint64_t *cols);

/* generic access used by the tests to check the parser against files written by libhdf5: numbers of any stored type
 * converted to f64 (dims gets up to 8 entries), fixed-length strings NUL-separated, link names NUL-separated */
int scanrs_h5_read_f64(const char *path, const char *dataset, double *out, uint64_t cap, uint64_t *dims, uint32_t *rank);
int scanrs_h5_read_strings(const char *path, const char *dataset, char *buf, uint64_t cap, uint64_t *n, uint64_t *bytes);
int scanrs_h5_member_names(const char *path, const char *group, char *buf, uint64_t cap, uint64_t *n, uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* SCANRS_AMD_H */
