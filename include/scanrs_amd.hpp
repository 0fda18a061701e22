// scanrs_amd.hpp — header-only C++ mirror of the reference's operator / solver surface over the C ABI
// (scanrs_amd.h). Same names, argument meaning and error behaviour as the Rust API it stands for:
//   sqz::AdaptiveMat / LowRankOffset      -> scanrs::AdaptiveMat   (sqz/src/mat.rs:34-42, low_rank_offset.rs:12-16)
//   scan_rs::normalization::*              -> scanrs::normalize ... (scan-rs/src/normalization.rs:11-213)
//   scan_rs::dim_red::{BkSvd,RandSvd,Irlba} -> scanrs::BkSvd ...   (scan-rs/src/dim_red/*.rs)
//   snoop::CancelProgress                  -> scanrs::Snoop         (snoop/src/lib.rs:20-58)
// `anyhow::Error` becomes scanrs::Error (code + the reference's message), `CancellationError` its subclass.
#pragma once
#include <array>
#include <atomic>
#include <cstdint>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "scanrs_amd.h"

namespace scanrs {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
struct CancellationError : Error { // snoop/src/lib.rs:5-18
    CancellationError() : Error(SCANRS_ERR_CANCELLED, "cancellation error") {}
};
inline void check(int code) {
    if (code == SCANRS_OK) return;
    if (code == SCANRS_ERR_CANCELLED) throw CancellationError();
    throw Error(code, scanrs_last_error());
}

enum class Storage : int { CSR = SCANRS_CSR, CSC = SCANRS_CSC };                       // sqz/src/mat.rs:45-65
enum class Normalization : int {                                                       // normalization.rs:11-28
    CellRanger = 0, CellRanger8, SeuratLog, BinomialDeviance, BinomialPearson, WithSizeFactors, LogTransform
};
enum class LogBase : int { E = SCANRS_FN_LN_1P, Two = SCANRS_FN_LOG2_1P, Ten = SCANRS_FN_LOG10_1P }; // :105-112

inline Normalization normalization_from_str(const std::string &s) { // impl FromStr, normalization.rs:30-43
    if (s == "cellranger") return Normalization::CellRanger;
    if (s == "cellranger8") return Normalization::CellRanger8;
    if (s == "seuratlog") return Normalization::SeuratLog;
    if (s == "binomialdeviance") return Normalization::BinomialDeviance;
    if (s == "binomialpearson") return Normalization::BinomialPearson;
    throw Error(SCANRS_ERR_ARGUMENT, "Normalization not recognized: " + s);
}

// row-major dense array, the stand-in for ndarray::Array2<f64>
struct Array2 {
    size_t rows = 0, cols = 0;
    std::vector<double> data;
    Array2() = default;
    Array2(size_t r, size_t c) : rows(r), cols(c), data(r * c, 0.0) {}
    double &operator()(size_t r, size_t c) { return data[r * cols + c]; }
    double operator()(size_t r, size_t c) const { return data[r * cols + c]; }
};

// snoop::CancelProgress: a cancel flag another thread may set + a progress sink
struct Snoop {
    std::atomic<uint8_t> cancelled{0};
    std::function<void(double)> on_progress;
    void cancel() { cancelled.store(1, std::memory_order_relaxed); }
    bool is_cancelled() const { return cancelled.load(std::memory_order_relaxed) != 0; }
};

struct PcaResult { // (u, d, v): dim_red/mod.rs:47
    Array2 u;
    std::vector<double> s;
    Array2 v;
};

enum class ExportMajor { Stored = SCANRS_EXPORT_STORED, Inner = SCANRS_EXPORT_INNER };

// The stored counts as AdaptiveVec encodings (scanrs_mat_to_adaptive[_major], scanrs_multi_to_adaptive): owns the host arenas and the
// table pointing into them
class AdaptiveExport {
    scanrs_adaptive_export *e_ = nullptr;

  public:
    AdaptiveExport() = default;
    explicit AdaptiveExport(scanrs_adaptive_export *e) : e_(e) {}
    AdaptiveExport(const AdaptiveExport &) = delete;
    AdaptiveExport &operator=(const AdaptiveExport &) = delete;
    AdaptiveExport(AdaptiveExport &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    AdaptiveExport &operator=(AdaptiveExport &&o) noexcept {
        if (this != &o) {
            scanrs_adaptive_export_free(e_);
            e_ = o.e_;
            o.e_ = nullptr;
        }
        return *this;
    }
    ~AdaptiveExport() { scanrs_adaptive_export_free(e_); }
    uint64_t n_vecs() const {
        uint64_t n = 0;
        check(scanrs_adaptive_export_info(e_, &n, nullptr, nullptr));
        return n;
    }
    uint64_t total_bytes() const { // sum of AdaptiveVec::mem_size
        uint64_t b = 0;
        check(scanrs_adaptive_export_info(e_, nullptr, &b, nullptr));
        return b;
    }
    std::array<uint64_t, 8> kind_counts() const { // D3, D4, D8, D16, V, S3, S4, S8
        std::array<uint64_t, 8> k{};
        check(scanrs_adaptive_export_info(e_, nullptr, nullptr, k.data()));
        return k;
    }
    // n_vecs() entries, valid while this object lives; what AdaptiveMat::from_adaptive_vecs / scanrs_mat_create_adaptive take
    const scanrs_adaptive_vec *vecs() const {
        const scanrs_adaptive_vec *v = nullptr;
        check(scanrs_adaptive_export_vecs(e_, &v));
        return v;
    }
    // scanrs_adaptive_export_multi_info: what MultiMat::to_adaptive did (slab_bounds n_shards + 1, moved n_shards x n_shards,
    // arena_bytes per shard). Error on an export of a single handle.
    struct MultiInfo {
        uint32_t n_shards = 0;
        std::vector<uint64_t> slab_bounds, moved, arena_bytes;
    };
    MultiInfo multi_info() const {
        MultiInfo m;
        check(scanrs_adaptive_export_multi_info(e_, &m.n_shards, nullptr, nullptr, nullptr));
        m.slab_bounds.resize(m.n_shards + 1);
        m.moved.resize((size_t)m.n_shards * m.n_shards);
        m.arena_bytes.resize(m.n_shards);
        check(scanrs_adaptive_export_multi_info(e_, nullptr, m.slab_bounds.data(), m.moved.data(), m.arena_bytes.data()));
        return m;
    }
};

// AdaptiveVec::choose_storage (vec.rs:1086-1131) on the host: (kind code, min_size)
inline std::pair<int, uint64_t> choose_storage(uint64_t len, const std::vector<uint32_t> &values) {
    int kind = 0;
    uint64_t min_size = 0;
    check(scanrs_host_choose_storage(len, values.data(), values.size(), &kind, &min_size));
    return {kind, min_size};
}

// Device-resident AdaptiveMat; plays LowRankOffset once an offset is installed.
class AdaptiveMat {
    scanrs_mat *h_ = nullptr;
    explicit AdaptiveMat(scanrs_mat *h) : h_(h) {}
    static scanrs_snoop snoop_of(Snoop *s) {
        scanrs_snoop sn;
        sn.cancel = s ? reinterpret_cast<const volatile uint8_t *>(&s->cancelled) : nullptr;
        sn.progress = [](void *ctx, double f) {
            auto *sp = static_cast<Snoop *>(ctx);
            if (sp && sp->on_progress) sp->on_progress(f);
        };
        sn.ctx = s;
        return sn;
    }

  public:
    AdaptiveMat() = default;
    AdaptiveMat(const AdaptiveMat &) = delete;
    AdaptiveMat &operator=(const AdaptiveMat &) = delete;
    AdaptiveMat(AdaptiveMat &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    AdaptiveMat &operator=(AdaptiveMat &&o) noexcept {
        if (this != &o) {
            scanrs_mat_free(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~AdaptiveMat() { scanrs_mat_free(h_); } // Drop
    scanrs_mat *raw() const { return h_; }

    // AdaptiveMat::from_csmat (mat.rs:92-124)
    static AdaptiveMat from_csmat(uint64_t rows, uint64_t cols, Storage storage, const uint64_t *indptr, const uint32_t *indices,
                                  const uint32_t *data) {
        scanrs_mat *h = nullptr;
        check(scanrs_mat_create(rows, cols, (int)storage, indptr, indices, data, &h));
        return AdaptiveMat(h);
    }
    // AdaptiveMat::new(rows, cols, storage, Vec<AdaptiveVec>) (mat.rs:68-90): the encoded vectors, decoded on the device
    static AdaptiveMat from_adaptive_vecs(uint64_t rows, uint64_t cols, Storage storage, const std::vector<scanrs_adaptive_vec> &vecs) {
        scanrs_mat *h = nullptr;
        check(scanrs_mat_create_adaptive(rows, cols, (int)storage, vecs.data(), vecs.size(), &h));
        return AdaptiveMat(h);
    }
    AdaptiveMat view() const { // mat.rs:242-245
        scanrs_mat *h = nullptr;
        check(scanrs_mat_view(h_, &h));
        return AdaptiveMat(h);
    }
    AdaptiveMat t() const { // mat.rs:262-270 / low_rank_offset.rs:60-65
        scanrs_mat *h = nullptr;
        check(scanrs_mat_t(h_, &h));
        return AdaptiveMat(h);
    }
    uint64_t rows() const { return shape().first; }
    uint64_t cols() const { return shape().second; }
    std::pair<uint64_t, uint64_t> shape() const {
        uint64_t r = 0, c = 0;
        check(scanrs_mat_shape(h_, &r, &c));
        return {r, c};
    }
    uint64_t nnz() const {
        uint64_t n = 0;
        check(scanrs_mat_nnz(h_, &n));
        return n;
    }
    // lazy maps (consume-and-return in the reference; in place here)
    AdaptiveMat &compose_scale_axis(int axis, const std::vector<double> &factors) {
        if (factors.size() != (axis == 0 ? rows() : cols())) throw Error(SCANRS_ERR_SHAPE, "Dimension mismatch");
        check(scanrs_mat_compose_scale_axis(h_, axis, factors.data()));
        return *this;
    }
    AdaptiveMat &apply(int scalar_fn) {
        check(scanrs_mat_apply(h_, scalar_fn));
        return *this;
    }
    AdaptiveMat &scale_and_center(int axis, const std::vector<double> *scaling = nullptr) { // mat.rs:986-1001
        check(scanrs_mat_scale_and_center(h_, axis, scaling ? scaling->data() : nullptr));
        return *this;
    }
    AdaptiveMat &center(int axis, const std::vector<double> *means = nullptr) {
        check(scanrs_mat_center(h_, axis, means ? means->data() : nullptr));
        return *this;
    }
    AdaptiveMat &scale(int axis, const std::vector<double> *stds = nullptr) {
        check(scanrs_mat_scale(h_, axis, stds ? stds->data() : nullptr));
        return *this;
    }
    // reductions
    std::vector<uint32_t> sum_axis_u32(int axis) const {
        std::vector<uint32_t> out(axis == 0 ? cols() : rows());
        check(scanrs_mat_sum_axis_u32(h_, axis, out.data()));
        return out;
    }
    std::vector<double> mean_axis(int axis) const {
        std::vector<double> out(axis == 0 ? cols() : rows());
        check(scanrs_mat_mean_axis(h_, axis, out.data()));
        return out;
    }
    std::pair<std::vector<double>, std::vector<double>> mean_var_axis(int axis) const { // mat.rs:285-330
        std::vector<double> mean(axis == 0 ? cols() : rows()), var(mean.size());
        check(scanrs_mat_mean_var_axis(h_, axis, mean.data(), var.data()));
        return {mean, var};
    }
    std::vector<double> var_axis(int axis) const { // mat.rs:409-411
        std::vector<double> out(axis == 0 ? cols() : rows());
        check(scanrs_mat_var_axis(h_, axis, out.data()));
        return out;
    }
    // statistics over a list of columns (mat.rs:279-282, 333-374, 414-583): strictly ascending indices. The u64 forms read the raw
    // counts (exact), the f64 forms the mapped values (bit-reproducible)
    std::vector<uint64_t> sum_rows_u64(const std::vector<uint64_t> &cols_) const { // mat.rs:449-481
        std::vector<uint64_t> out(rows());
        check(scanrs_mat_sum_rows_u64(h_, cols_.data(), cols_.size(), out.data()));
        return out;
    }
    std::vector<double> sum_rows(const std::vector<uint64_t> &cols_) const {
        std::vector<double> out(rows());
        check(scanrs_mat_sum_rows_f64(h_, cols_.data(), cols_.size(), out.data()));
        return out;
    }
    std::vector<uint64_t> sum_cols_u64(const std::vector<uint64_t> &cols_) const { // mat.rs:414-446: one entry per listed column
        std::vector<uint64_t> out(cols_.size());
        check(scanrs_mat_sum_cols_u64(h_, cols_.data(), cols_.size(), out.data()));
        return out;
    }
    std::vector<double> sum_cols(const std::vector<uint64_t> &cols_) const {
        std::vector<double> out(cols_.size());
        check(scanrs_mat_sum_cols_f64(h_, cols_.data(), cols_.size(), out.data()));
        return out;
    }
    // sum_rows_dual / sum_rows_dual_with_cancellation (mat.rs:484-583): both lists in one walk; they may overlap
    std::pair<std::vector<uint64_t>, std::vector<uint64_t>> sum_rows_dual_u64(const std::vector<uint64_t> &cols1, const std::vector<uint64_t> &cols2,
                                                                            Snoop *snoop = nullptr) const {
        std::vector<uint64_t> a(rows()), b(rows());
        scanrs_snoop sn = snoop_of(snoop);
        check(scanrs_mat_sum_rows_dual_u64(h_, cols1.data(), cols1.size(), cols2.data(), cols2.size(), snoop ? &sn : nullptr, a.data(), b.data()));
        return {a, b};
    }
    std::pair<std::vector<double>, std::vector<double>> sum_rows_dual(const std::vector<uint64_t> &cols1, const std::vector<uint64_t> &cols2,
                                                                      Snoop *snoop = nullptr) const {
        std::vector<double> a(rows()), b(rows());
        scanrs_snoop sn = snoop_of(snoop);
        check(scanrs_mat_sum_rows_dual_f64(h_, cols1.data(), cols1.size(), cols2.data(), cols2.size(), snoop ? &sn : nullptr, a.data(), b.data()));
        return {a, b};
    }
    std::vector<double> mean_rows(const std::vector<uint64_t> &cols_) const { // mat.rs:279-282
        std::vector<double> out(rows());
        check(scanrs_mat_mean_rows(h_, cols_.data(), cols_.size(), out.data()));
        return out;
    }
    std::pair<std::vector<double>, std::vector<double>> mean_var_rows(const std::vector<uint64_t> &cols_) const { // mat.rs:333-374
        std::vector<double> mean(rows()), var(rows());
        check(scanrs_mat_mean_var_rows(h_, cols_.data(), cols_.size(), mean.data(), var.data()));
        return {mean, var};
    }
    // Dot impls: self.dot(rhs) and lhs.dot(self)
    Array2 dot(const Array2 &rhs) const {
        if (rhs.rows != cols()) throw Error(SCANRS_ERR_SHAPE, "Dimension mismatch"); // prod.rs:41
        Array2 out(rows(), rhs.cols);
        check(scanrs_mat_dot(h_, rhs.data.data(), (uint32_t)rhs.cols, out.data.data()));
        return out;
    }
    Array2 rdot(const Array2 &lhs) const {
        if (lhs.cols != rows()) throw Error(SCANRS_ERR_SHAPE, "Dimension mismatch");
        Array2 out(lhs.rows, cols());
        check(scanrs_mat_rdot(h_, lhs.data.data(), (uint32_t)lhs.rows, out.data.data()));
        return out;
    }
    // select_rows / select_cols (mat.rs:1004-1071): any order, repeats allowed; identity map, no offset, not sharded
    AdaptiveMat select_rows(const std::vector<uint64_t> &idx) const {
        scanrs_mat *h = nullptr;
        check(scanrs_mat_select_rows(h_, idx.data(), idx.size(), &h));
        return AdaptiveMat(h);
    }
    AdaptiveMat select_cols(const std::vector<uint64_t> &idx) const {
        scanrs_mat *h = nullptr;
        check(scanrs_mat_select_cols(h_, idx.data(), idx.size(), &h));
        return AdaptiveMat(h);
    }
    // partition_on_thresholds (mat.rs:766-888): (filtered, residual, selected_rows, selected_cols); nullptr = None
    struct Partition;
    Partition partition_on_thresholds(const double *row_threshold, const double *col_threshold) const;
    Partition partition_on_threshold(double threshold) const;
    // The collective forms for a sharded handle (scanrs_mat_*_sharded): every rank calls them with the same arguments; lists along
    // the sharded dimension span the whole matrix (a selection list there must not descend). The results are bound as this rank of
    // the same world. On an unsharded handle they are the plain calls.
    struct ShardInfo {
        uint32_t rank = 0, world = 1;
        uint64_t outer_begin = 0, outer_global = 0;
    };
    ShardInfo shard_info() const {
        ShardInfo i;
        check(scanrs_mat_shard_info(h_, &i.rank, &i.world, &i.outer_begin, &i.outer_global));
        return i;
    }
    AdaptiveMat select_rows_sharded(const std::vector<uint64_t> &idx) const {
        scanrs_mat *h = nullptr;
        check(scanrs_mat_select_rows_sharded(h_, idx.data(), idx.size(), &h));
        return AdaptiveMat(h);
    }
    AdaptiveMat select_cols_sharded(const std::vector<uint64_t> &idx) const {
        scanrs_mat *h = nullptr;
        check(scanrs_mat_select_cols_sharded(h_, idx.data(), idx.size(), &h));
        return AdaptiveMat(h);
    }
    Partition partition_on_thresholds_sharded(const double *row_threshold, const double *col_threshold) const;
    // to_csmat of the stored counts (mat.rs:207-241) in the handle's storage flag
    struct CsMat {
        int storage = SCANRS_CSR;
        uint64_t rows = 0, cols = 0;
        std::vector<uint64_t> indptr;
        std::vector<uint32_t> indices, data;
    };
    CsMat to_csmat() const {
        CsMat c;
        check(scanrs_mat_storage(h_, &c.storage));
        c.rows = rows();
        c.cols = cols();
        c.indptr.resize((c.storage == SCANRS_CSR ? c.rows : c.cols) + 1);
        c.indices.resize(nnz());
        c.data.resize(nnz());
        check(scanrs_mat_to_csmat(h_, c.indptr.data(), c.indices.data(), c.data.data()));
        return c;
    }
    // AdaptiveMat::from_csmat backwards (mat.rs:92-124, vec.rs:1086-1160): one encoded AdaptiveVec per outer vector of the stored
    // counts, made on the device. force_kind -1: choose_storage; 0..7: that encoding for every vector
    AdaptiveExport to_adaptive(int force_kind = -1) const {
        scanrs_adaptive_export *e = nullptr;
        check(scanrs_mat_to_adaptive(h_, force_kind, &e));
        return AdaptiveExport(e);
    }
    // major Inner: one vector per INNER position, from the handle's transposed copy (the table from_adaptive_vecs takes with the
    // OTHER storage flag); refused on a sharded handle
    AdaptiveExport to_adaptive(int force_kind, ExportMajor major) const {
        scanrs_adaptive_export *e = nullptr;
        check(scanrs_mat_to_adaptive_major(h_, (int)major, force_kind, &e));
        return AdaptiveExport(e);
    }
    Array2 to_dense() const {
        Array2 out(rows(), cols());
        check(scanrs_mat_to_dense(h_, out.data.data()));
        return out;
    }
};

struct AdaptiveMat::Partition {
    AdaptiveMat filtered, residual;
    std::vector<uint64_t> selected_rows, selected_cols;
};
inline AdaptiveMat::Partition AdaptiveMat::partition_on_thresholds(const double *row_threshold, const double *col_threshold) const {
    Partition p;
    p.selected_rows.resize(rows());
    p.selected_cols.resize(cols());
    uint64_t nr = 0, nc = 0;
    scanrs_mat *f = nullptr, *r = nullptr;
    check(scanrs_mat_partition_on_thresholds(h_, row_threshold, col_threshold, &f, &r, p.selected_rows.data(), &nr, p.selected_cols.data(), &nc));
    p.filtered = AdaptiveMat(f);
    p.residual = AdaptiveMat(r);
    p.selected_rows.resize(nr);
    p.selected_cols.resize(nc);
    return p;
}
inline AdaptiveMat::Partition AdaptiveMat::partition_on_threshold(double threshold) const { return partition_on_thresholds(&threshold, &threshold); }
inline AdaptiveMat::Partition AdaptiveMat::partition_on_thresholds_sharded(const double *row_threshold, const double *col_threshold) const {
    const ShardInfo si = shard_info();
    int storage = SCANRS_CSR;
    check(scanrs_mat_storage(h_, &storage));
    Partition p; // the lists of the sharded dimension have outer_global entries: the rows of a CSR handle, the columns of a CSC one
    p.selected_rows.resize((storage == SCANRS_CSR ? si.outer_global : rows()) + 1); // (+ 1: never a null array)
    p.selected_cols.resize((storage == SCANRS_CSR ? cols() : si.outer_global) + 1);
    uint64_t nr = 0, nc = 0;
    scanrs_mat *f = nullptr, *r = nullptr;
    check(scanrs_mat_partition_on_thresholds_sharded(h_, row_threshold, col_threshold, &f, &r, p.selected_rows.data(), &nr, p.selected_cols.data(), &nc));
    p.filtered = AdaptiveMat(f);
    p.residual = AdaptiveMat(r);
    p.selected_rows.resize(nr);
    p.selected_cols.resize(nc);
    return p;
}

// normalize(mat, norm) -> LowRankOffset (normalization.rs:46-69); consumes `mat` like the reference.
inline AdaptiveMat normalize(AdaptiveMat mat, Normalization norm) {
    check(scanrs_normalize(mat.raw(), (int)norm, nullptr));
    return mat;
}
inline AdaptiveMat normalize_with_size_factor(AdaptiveMat mat, Normalization norm, const std::vector<uint32_t> *size_factors) {
    if (size_factors && size_factors->size() != mat.cols())
        throw Error(SCANRS_ERR_SHAPE, "Size of the size factor and matrix columns dont match.");
    check(scanrs_normalize(mat.raw(), (int)norm, size_factors ? size_factors->data() : nullptr));
    return mat;
}
inline AdaptiveMat binom_deviance_resid(AdaptiveMat mat) { return normalize(std::move(mat), Normalization::BinomialDeviance); }
inline AdaptiveMat binom_pearson_resid(AdaptiveMat mat) { return normalize(std::move(mat), Normalization::BinomialPearson); }

// nn::knn (scan-rs/src/nn.rs:38-57): k nearest other rows of the cells x d matrix, nearest first
inline std::vector<uint32_t> knn(const Array2 &v, size_t k) {
    std::vector<uint32_t> out(v.rows * k);
    check(scanrs_knn(v.data.data(), v.rows, (uint32_t)v.cols, (uint32_t)k, out.data()));
    return out;
}

namespace detail {
inline void progress_tramp(void *ctx, double f) {
    auto *s = static_cast<Snoop *>(ctx);
    if (s->on_progress) s->on_progress(f);
}
inline scanrs_snoop make_snoop(Snoop *s) {
    scanrs_snoop sn;
    sn.cancel = reinterpret_cast<const volatile uint8_t *>(&s->cancelled);
    sn.progress = &progress_tramp;
    sn.ctx = s;
    return sn;
}
} // namespace detail

// trait Pca<T, N> (dim_red/mod.rs:103-111): run_pca_cancellable / run_pca
struct BkSvd { // dim_red/bk_svd.rs:16-39
    double k_multiplier = 2.0;
    size_t n_iter = 5;
    PcaResult run_pca_cancellable(const AdaptiveMat &m, size_t k, Snoop *snoop) const {
        PcaResult r{Array2(m.rows(), k), std::vector<double>(k), Array2(m.cols(), k)};
        scanrs_snoop sn;
        if (snoop) sn = detail::make_snoop(snoop);
        check(scanrs_pca_bk(m.raw(), (uint32_t)k, k_multiplier, (uint32_t)n_iter, 0, nullptr, snoop ? &sn : nullptr,
                            r.u.data.data(), r.s.data(), r.v.data.data()));
        return r;
    }
    PcaResult run_pca(const AdaptiveMat &m, size_t k) const { return run_pca_cancellable(m, k, nullptr); }
};
struct RandSvd { // dim_red/rand_svd.rs:13-35
    double l_multiplier = 10.0;
    size_t n_iter = 2;
    PcaResult run_pca(const AdaptiveMat &m, size_t k) const {
        PcaResult r{Array2(m.rows(), k), std::vector<double>(k), Array2(m.cols(), k)};
        check(scanrs_pca_rand(m.raw(), (uint32_t)k, l_multiplier, (uint32_t)n_iter, 0, nullptr, r.u.data.data(), r.s.data(),
                              r.v.data.data()));
        return r;
    }
};
struct Irlba { // dim_red/irlba.rs:36-57
    double tol = 0.0001;
    size_t max_iter = 50;
    PcaResult run_pca_cancellable(const AdaptiveMat &m, size_t k, Snoop *snoop) const {
        PcaResult r{Array2(m.rows(), k), std::vector<double>(k), Array2(m.cols(), k)};
        scanrs_snoop sn;
        if (snoop) sn = detail::make_snoop(snoop);
        uint32_t mprod = 0;
        check(scanrs_pca_irlba(m.raw(), (uint32_t)k, tol, (uint32_t)max_iter, nullptr, snoop ? &sn : nullptr, r.u.data.data(),
                               r.s.data(), r.v.data.data(), &mprod));
        return r;
    }
    PcaResult run_pca(const AdaptiveMat &m, size_t k) const { return run_pca_cancellable(m, k, nullptr); }
};

// PcaResult left in device memory by the last BkSvd / RandSvd call on `m` (scanrs_pca_result_device): for device consumers
struct PcaResultDevice {
    const double *d_u = nullptr, *d_v = nullptr; // rows x k, cols x k, row-major with leading dimensions ld_u / ld_v (elements)
    uint32_t ld_u = 0, ld_v = 0, k = 0;
};
inline PcaResultDevice pca_result_device(const AdaptiveMat &m) {
    PcaResultDevice r;
    check(scanrs_pca_result_device(m.raw(), &r.d_u, &r.ld_u, &r.d_v, &r.ld_v, &r.k));
    return r;
}
// nn::knn on scores that are already in device memory
inline std::vector<uint32_t> knn_device(const double *d_points, size_t n, uint32_t ld, uint32_t d, size_t k) {
    std::vector<uint32_t> out(n * k);
    check(scanrs_knn_device(d_points, n, ld, d, (uint32_t)k, out.data()));
    return out;
}

// The single-process multi-GPU form (scanrs_multi_*): one object for the whole matrix, sharded by the library over
// `n_shards` devices; normalize + run_pca as on a single handle, results for the whole matrix.
class MultiMat {
    scanrs_multi *h_ = nullptr;
    size_t rows_ = 0, cols_ = 0;

  public:
    MultiMat(size_t rows, size_t cols, int storage, const uint64_t *indptr, const uint32_t *indices, const uint32_t *values,
             uint32_t n_shards, const int *devices = nullptr)
        : rows_(rows), cols_(cols) {
        check(scanrs_multi_create(rows, cols, storage, indptr, indices, values, n_shards, devices, &h_));
    }
    MultiMat() = default;
    // takes over a handle (the results of select_rows / select_cols / partition_on_thresholds)
    explicit MultiMat(scanrs_multi *h) : h_(h) {
        if (!h) return;
        uint64_t r = 0, c = 0;
        check(scanrs_multi_shape(h, &r, &c, nullptr, nullptr));
        rows_ = r;
        cols_ = c;
    }
    // Cell-sharded from feature-major input: the matrix in the reference's own orientation (genes x cells CSR, one vector per
    // gene), its INNER dimension sharded over the devices. The result has the same rows x cols and the other storage flag and equals
    // MultiMat(host-transposed triplet) bit for bit; nothing is transposed on the host, every nonzero is uploaded once.
    // scanrs_multi_create_inner (AdaptiveMat::from_csmat, sqz/src/mat.rs:92-124)
    static MultiMat from_csmat_inner(size_t rows, size_t cols, int storage, const uint64_t *indptr, const uint32_t *indices, const uint32_t *values,
                                     uint32_t n_shards, const int *devices = nullptr) {
        scanrs_multi *h = nullptr;
        check(scanrs_multi_create_inner(rows, cols, storage, indptr, indices, values, n_shards, devices, &h));
        return MultiMat(h);
    }
    // scanrs_multi_create_adaptive_inner (AdaptiveMat::new(rows, cols, storage, Vec<AdaptiveVec>), mat.rs:68-90): one entry per outer vector
    static MultiMat from_adaptive_vecs_inner(size_t rows, size_t cols, int storage, const scanrs_adaptive_vec *vecs, size_t n_vecs, uint32_t n_shards,
                                             const int *devices = nullptr) {
        scanrs_multi *h = nullptr;
        check(scanrs_multi_create_adaptive_inner(rows, cols, storage, vecs, n_vecs, n_shards, devices, &h));
        return MultiMat(h);
    }
    // scanrs_multi_create_from_file (cmd.rs:61-70): read_adaptive_csr_matrix for ".h5" (hdf5-io/src/matrix.rs:119-192), load_mtx otherwise (mtx.rs:10-51)
    static MultiMat from_file(const std::string &path, uint32_t n_shards, const int *devices = nullptr, const char *retain_feature_like = nullptr,
                              int64_t shrink_row = -1) {
        scanrs_multi *h = nullptr;
        check(scanrs_multi_create_from_file(path.c_str(), retain_feature_like, shrink_row, n_shards, devices, &h, nullptr));
        return MultiMat(h);
    }
    uint32_t n_shards() const {
        uint32_t n = 0;
        check(scanrs_multi_n_shards(h_, &n));
        return n;
    }
    // what an inner-sharding constructor did (scanrs_multi_create_info): the slabs of the outer vectors, moved[s * n + d] = stored entries
    // of slab s in shard d's range, bytes uploaded per shard. Error on a MultiMat that no such constructor made.
    struct CreateInfo {
        std::vector<uint64_t> slab_bounds, moved, uploaded_bytes;
    };
    CreateInfo create_info() const {
        const uint32_t n = n_shards();
        CreateInfo c{std::vector<uint64_t>(n + 1), std::vector<uint64_t>((size_t)n * n), std::vector<uint64_t>(n)};
        check(scanrs_multi_create_info(h_, c.slab_bounds.data(), c.moved.data(), c.uploaded_bytes.data()));
        return c;
    }
    MultiMat(const MultiMat &) = delete;
    MultiMat &operator=(const MultiMat &) = delete;
    MultiMat(MultiMat &&o) noexcept : h_(o.h_), rows_(o.rows_), cols_(o.cols_) { o.h_ = nullptr; }
    MultiMat &operator=(MultiMat &&o) noexcept {
        if (this != &o) {
            scanrs_multi_free(h_);
            h_ = o.h_;
            rows_ = o.rows_;
            cols_ = o.cols_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~MultiMat() { scanrs_multi_free(h_); }
    size_t rows() const { return rows_; }
    size_t cols() const { return cols_; }
    scanrs_multi *raw() const { return h_; }
    uint64_t nnz() const {
        uint64_t n = 0;
        check(scanrs_multi_shape(h_, nullptr, nullptr, &n, nullptr));
        return n;
    }
    // the whole matrix, shards concatenated (scanrs_multi_to_csmat)
    AdaptiveMat::CsMat to_csmat() const {
        AdaptiveMat::CsMat c;
        uint64_t n = 0;
        check(scanrs_multi_shape(h_, &c.rows, &c.cols, &n, &c.storage));
        c.indptr.resize((c.storage == SCANRS_CSR ? c.rows : c.cols) + 1);
        c.indices.resize(n);
        c.data.resize(n);
        check(scanrs_multi_to_csmat(h_, c.indptr.data(), c.indices.data(), c.data.data()));
        return c;
    }
    // select_rows / select_cols / partition_on_thresholds over the shards (scanrs_multi_select_*): new MultiMat objects on
    // the same devices, shards not rebalanced. A list along the sharded dimension must not descend.
    MultiMat select_rows(const std::vector<uint64_t> &idx) const {
        scanrs_multi *h = nullptr;
        check(scanrs_multi_select_rows(h_, idx.data(), idx.size(), &h));
        return MultiMat(h);
    }
    MultiMat select_cols(const std::vector<uint64_t> &idx) const {
        scanrs_multi *h = nullptr;
        check(scanrs_multi_select_cols(h_, idx.data(), idx.size(), &h));
        return MultiMat(h);
    }
    // Outer vectors move between shards. gather_outer (scanrs_multi_gather_outer): the outer vectors idx of the whole matrix
    // in list order - any order, repeats allowed - as a freshly balanced MultiMat over n_shards shards on `devices` (null: 0 .. n_shards-1);
    // it equals MultiMat(selected triplet) bit for bit, and no nonzero crosses the host link. rebalance (scanrs_multi_rebalance): the
    // identity list; n_shards = 0: as many shards as this one, on its devices.
    MultiMat gather_outer(const std::vector<uint64_t> &idx, uint32_t n_shards, const int *devices = nullptr) const {
        scanrs_multi *h = nullptr;
        check(scanrs_multi_gather_outer(h_, idx.data(), idx.size(), n_shards, devices, &h));
        return MultiMat(h);
    }
    MultiMat rebalance(uint32_t n_shards = 0, const int *devices = nullptr) const {
        scanrs_multi *h = nullptr;
        check(scanrs_multi_rebalance(h_, n_shards, devices, &h));
        return MultiMat(h);
    }
    // scanrs_multi_balance: the nonzeros of every shard and max / mean of them
    struct Balance {
        std::vector<uint64_t> shard_nnz;
        double imbalance = 1.0;
    };
    Balance balance() const {
        Balance b{std::vector<uint64_t>(n_shards()), 1.0};
        check(scanrs_multi_balance(h_, b.shard_nnz.data(), &b.imbalance));
        return b;
    }
    // scanrs_multi_gather_info: what gather_outer / rebalance did. moved[s * n_shards + d]: nonzeros from source shard s to shard d;
    // host_bytes: what crossed the host link per shard (metadata only). Error on a MultiMat these calls did not make.
    struct GatherInfo {
        uint32_t n_src = 0;
        std::vector<uint64_t> bounds, moved, host_bytes;
    };
    GatherInfo gather_info() const {
        const uint32_t n = n_shards();
        GatherInfo g;
        check(scanrs_multi_gather_info(h_, &g.n_src, nullptr, nullptr, nullptr));
        g.bounds.resize(n + 1);
        g.moved.resize((size_t)g.n_src * n);
        g.host_bytes.resize(n);
        check(scanrs_multi_gather_info(h_, nullptr, g.bounds.data(), g.moved.data(), g.host_bytes.data()));
        return g;
    }
    // scanrs_multi_to_adaptive: the whole matrix as one table of AdaptiveVec encodings. Stored: one per outer vector in global order;
    // Inner (the inverse of from_adaptive_vecs_inner): one per inner position, each spanning all shards
    AdaptiveExport to_adaptive(int force_kind = -1, ExportMajor major = ExportMajor::Stored) const {
        scanrs_adaptive_export *e = nullptr;
        check(scanrs_multi_to_adaptive(h_, (int)major, force_kind, &e));
        return AdaptiveExport(e);
    }
    struct Partition;
    Partition partition_on_thresholds(const double *row_threshold, const double *col_threshold) const;
    Partition partition_on_threshold(double threshold) const;
    // payload bytes of the sum all-reduces that went through shard i's communicator so far (scanrs_multi_comm_info)
    uint64_t allreduce_bytes(uint32_t i = 0) const {
        uint64_t b = 0;
        check(scanrs_multi_comm_info(h_, i, nullptr, nullptr, nullptr, &b));
        return b;
    }
    void normalize(Normalization norm) { check(scanrs_multi_normalize(h_, (int)norm, nullptr)); }
    PcaResult run_pca(const BkSvd &cfg, size_t k) {
        PcaResult r{Array2(rows_, k), std::vector<double>(k), Array2(cols_, k)};
        check(scanrs_multi_pca_bk(h_, (uint32_t)k, cfg.k_multiplier, (uint32_t)cfg.n_iter, 0, nullptr, nullptr, r.u.data.data(),
                                  r.s.data(), r.v.data.data()));
        return r;
    }
};

struct MultiMat::Partition {
    MultiMat filtered, residual;
    std::vector<uint64_t> selected_rows, selected_cols;
};
inline MultiMat::Partition MultiMat::partition_on_thresholds(const double *row_threshold, const double *col_threshold) const {
    Partition p;
    p.selected_rows.resize(rows_ + 1); // (+ 1: never a null array)
    p.selected_cols.resize(cols_ + 1);
    uint64_t nr = 0, nc = 0;
    scanrs_multi *f = nullptr, *r = nullptr;
    check(scanrs_multi_partition_on_thresholds(h_, row_threshold, col_threshold, &f, &r, p.selected_rows.data(), &nr, p.selected_cols.data(), &nc));
    p.filtered = MultiMat(f);
    p.residual = MultiMat(r);
    p.selected_rows.resize(nr);
    p.selected_cols.resize(nc);
    return p;
}
inline MultiMat::Partition MultiMat::partition_on_threshold(double threshold) const { return partition_on_thresholds(&threshold, &threshold); }

// scanrs_host_plan_inner (host only, no device): the plan of the inner-sharding constructors for a feature-major triplet
struct InnerPlan {
    std::vector<uint64_t> slab_bounds, bounds, moved; // world + 1, world + 1, world x world
};
inline InnerPlan host_plan_inner(const uint64_t *indptr, const uint32_t *indices, uint64_t n_outer, uint64_t n_inner, uint32_t world) {
    InnerPlan p{std::vector<uint64_t>(world + 1), std::vector<uint64_t>(world + 1), std::vector<uint64_t>((size_t)world * world + 1)};
    check(scanrs_host_plan_inner(indptr, indices, n_outer, n_inner, world, p.slab_bounds.data(), p.bounds.data(), p.moved.data()));
    p.moved.resize((size_t)world * world);
    return p;
}

// scanrs_host_plan_export (host only, no device): the plan of MultiMat::to_adaptive(.., ExportMajor::Inner) from counts (n_src x n_inner)
struct ExportPlan {
    std::vector<uint64_t> indptr, slab_bounds, moved; // n_inner + 1, n_dst + 1, n_src x n_dst
};
inline ExportPlan host_plan_export(const std::vector<uint64_t> &counts, uint32_t n_src, uint64_t n_inner, uint32_t n_dst) {
    ExportPlan p{std::vector<uint64_t>(n_inner + 1), std::vector<uint64_t>(n_dst + 1), std::vector<uint64_t>((size_t)n_src * n_dst + 1)};
    check(scanrs_host_plan_export(counts.data(), n_src, n_inner, n_dst, p.indptr.data(), p.slab_bounds.data(), p.moved.data()));
    p.moved.resize((size_t)n_src * n_dst);
    return p;
}

// scanrs_host_plan_gather (host only, no device): the plan of MultiMat::gather_outer / rebalance from the source's global indptr, its
// shard bounds and the list
struct GatherPlan {
    std::vector<uint64_t> indptr, bounds, moved; // n_idx + 1 (the selected matrix's), n_dst + 1, n_src x n_dst
};
inline GatherPlan host_plan_gather(const uint64_t *indptr, uint64_t n_outer, const std::vector<uint64_t> &src_bounds, const std::vector<uint64_t> &idx,
                                   uint32_t n_dst) {
    const uint32_t n_src = src_bounds.empty() ? 0u : (uint32_t)(src_bounds.size() - 1);
    GatherPlan p{std::vector<uint64_t>(idx.size() + 1), std::vector<uint64_t>(n_dst + 1), std::vector<uint64_t>((size_t)n_src * n_dst + 1)};
    check(scanrs_host_plan_gather(indptr, n_outer, src_bounds.data(), n_src, idx.data(), idx.size(), n_dst, p.indptr.data(), p.bounds.data(),
                                  p.moved.data()));
    p.moved.resize((size_t)n_src * n_dst);
    return p;
}

// ---- hdf5-io crate (hdf5-io/src/matrix.rs, analysis.rs): 10x files -> host arrays, parsed by the library itself ----
namespace hdf5_io {
static const char *const FEATURE_TYPE_GENE_EXPRESSION = "Gene Expression"; // matrix.rs:14

// GenericFeatureBarcodeMatrix / MatrixMetadata (scan-types/src/matrix.rs:8-15) with the matrix as host arrays
struct FeatureBarcodeMatrix {
    std::string name;
    std::vector<std::string> barcodes, feature_ids, feature_names, feature_types;
    Storage storage = Storage::CSC;
    uint64_t rows = 0, cols = 0, nnz = 0;
    std::vector<uint64_t> indptr; // empty for read_matrix_metadata
    std::vector<uint32_t> indices, values;
    std::vector<uint64_t> removed_features; // ascending (the BTreeSet of the reference)
    AdaptiveMat to_device() const { return AdaptiveMat::from_csmat(rows, cols, storage, indptr.data(), indices.data(), values.data()); }
    // over n_shards devices with the barcodes sharded (MultiMat::from_csmat_inner: the matrix is feature-major, its inner dimension is cut)
    MultiMat to_devices(uint32_t n_shards, const int *devices = nullptr) const {
        return MultiMat::from_csmat_inner(rows, cols, (int)storage, indptr.data(), indices.data(), values.data(), n_shards, devices);
    }
};

namespace detail {
inline FeatureBarcodeMatrix take(scanrs_h5_matrix *h) {
    struct Free {
        scanrs_h5_matrix *h;
        ~Free() { scanrs_h5_matrix_free(h); }
    } guard{h};
    FeatureBarcodeMatrix m;
    int storage = 0;
    check(scanrs_h5_matrix_shape(h, &m.rows, &m.cols, &m.nnz, &storage));
    m.storage = (Storage)storage;
    auto strings = [&](int what) {
        uint64_t n = 0;
        check(scanrs_h5_matrix_n_strings(h, what, &n));
        std::vector<std::string> v(n);
        for (uint64_t i = 0; i < n; i++) v[i] = scanrs_h5_matrix_string(h, what, i);
        return v;
    };
    m.barcodes = strings(0);
    m.feature_ids = strings(1);
    m.feature_names = strings(2);
    m.feature_types = strings(3);
    m.name = strings(4)[0];
    const uint64_t *ip = nullptr, *rem = nullptr;
    const uint32_t *ix = nullptr, *vv = nullptr;
    check(scanrs_h5_matrix_arrays(h, &ip, &ix, &vv));
    if (ip) {
        const uint64_t n_outer = m.storage == Storage::CSR ? m.rows : m.cols;
        m.indptr.assign(ip, ip + n_outer + 1);
        m.indices.assign(ix, ix + m.nnz);
        m.values.assign(vv, vv + m.nnz);
    }
    uint64_t n_rem = 0;
    check(scanrs_h5_matrix_removed(h, &rem, &n_rem));
    m.removed_features.assign(rem, rem + n_rem);
    return m;
}
inline std::vector<std::string> unpack(const std::vector<char> &buf, uint64_t n) {
    std::vector<std::string> out;
    const char *p = buf.data();
    for (uint64_t i = 0; i < n; i++) {
        out.emplace_back(p);
        p += out.back().size() + 1;
    }
    return out;
}
} // namespace detail

inline FeatureBarcodeMatrix read_csc_matrix(const std::string &path) { // matrix.rs:56-97
    scanrs_h5_matrix *h = nullptr;
    check(scanrs_h5_read_csc_matrix(path.c_str(), &h));
    return detail::take(h);
}
// matrix.rs:129-199; retain_feature_like == nullptr: None; shrink_row < 0: None
inline FeatureBarcodeMatrix read_adaptive_csr_matrix(const std::string &path, const char *retain_feature_like = nullptr, int64_t shrink_row = -1) {
    scanrs_h5_matrix *h = nullptr;
    check(scanrs_h5_read_adaptive_csr_matrix(path.c_str(), retain_feature_like, shrink_row, &h));
    return detail::take(h);
}
inline FeatureBarcodeMatrix read_matrix_metadata(const std::string &path, const char *retain_feature_like = nullptr) { // matrix.rs:17-54
    scanrs_h5_matrix *h = nullptr;
    check(scanrs_h5_read_matrix_metadata(path.c_str(), retain_feature_like, &h));
    return detail::take(h);
}
inline std::vector<uint32_t> read_umi_counts_from_matrix(const std::string &path) { // matrix.rs:270-299
    uint64_t n = 0;
    check(scanrs_h5_read_umi_counts(path.c_str(), nullptr, 0, &n));
    std::vector<uint32_t> out(n);
    check(scanrs_h5_read_umi_counts(path.c_str(), out.data(), n, &n));
    return out;
}
inline std::vector<std::string> get_clustering_keys(const std::string &analysis_h5) { // analysis.rs:38-41
    uint64_t n = 0, bytes = 0;
    check(scanrs_h5_get_clustering_keys(analysis_h5.c_str(), nullptr, 0, &n, &bytes));
    std::vector<char> buf(bytes + 1);
    check(scanrs_h5_get_clustering_keys(analysis_h5.c_str(), buf.data(), bytes, &n, &bytes));
    return detail::unpack(buf, n);
}
inline std::pair<uint16_t, std::vector<int16_t>> get_clustering(const std::string &analysis_h5, const std::string &key) { // analysis.rs:5-20
    uint16_t nc = 0;
    uint64_t n = 0;
    check(scanrs_h5_get_clustering(analysis_h5.c_str(), key.c_str(), &nc, nullptr, 0, &n));
    std::vector<int16_t> c(n);
    check(scanrs_h5_get_clustering(analysis_h5.c_str(), key.c_str(), &nc, c.data(), n, &n));
    return {nc, std::move(c)};
}
inline Array2 get_differential_expression(const std::string &analysis_h5, const std::string &key) { // analysis.rs:23-36
    uint64_t r = 0, c = 0;
    check(scanrs_h5_get_differential_expression(analysis_h5.c_str(), key.c_str(), nullptr, 0, &r, &c));
    Array2 out(r, c);
    check(scanrs_h5_get_differential_expression(analysis_h5.c_str(), key.c_str(), out.data.data(), r * c, &r, &c));
    return out;
}
} // namespace hdf5_io

namespace diff_exp {
// sSeq differential expression (diff-exp/src/diff_exp.rs): genes = rows, cells = cols of the handle; raw u32 counts
constexpr uint64_t BIG_COUNT_DEFAULT = 900;
constexpr double ZETA_QUINTILE_DEFAULT = 0.995;
enum class NbExactBackend : int { LogSpace = SCANRS_NB_EXACT_LOGSPACE, Ratio = SCANRS_NB_EXACT_RATIO }; // dist.rs:52-68
struct SSeqParams { // diff_exp.rs:19-40
    uint32_t num_cells = 0, num_genes = 0;
    std::vector<double> size_factors, gene_means, gene_variances;
    std::vector<uint8_t> use_genes;
    std::vector<double> gene_moment_phi;
    double zeta_hat = 0.0, delta = 0.0;
    std::vector<double> gene_phi;
};
struct DiffExpResult { // diff_exp.rs:42-65 (genes_tested / common_* are the params' use_genes / gene_means / gene_phi)
    std::vector<uint64_t> sums_in, sums_out;
    std::vector<double> normalized_mean_in, normalized_mean_out, p_values, adjusted_p_values, log2_fold_change;
};
inline SSeqParams compute_sseq_params(const AdaptiveMat &m, double zeta_quintile = ZETA_QUINTILE_DEFAULT,
                                      const std::vector<uint64_t> *cell_indices = nullptr, const std::vector<double> *umi_counts = nullptr) {
    SSeqParams p;
    const uint64_t g = m.rows(), c = m.cols();
    p.num_genes = (uint32_t)g;
    p.num_cells = (uint32_t)(cell_indices ? cell_indices->size() : c);
    p.size_factors.resize(c);
    p.gene_means.resize(g);
    p.gene_variances.resize(g);
    p.use_genes.resize(g);
    p.gene_moment_phi.resize(g);
    p.gene_phi.resize(g);
    check(scanrs_sseq_params(m.raw(), zeta_quintile, cell_indices ? cell_indices->data() : nullptr, cell_indices ? cell_indices->size() : 0,
                             umi_counts ? umi_counts->data() : nullptr, p.size_factors.data(), p.gene_means.data(), p.gene_variances.data(),
                             p.use_genes.data(), p.gene_moment_phi.data(), &p.zeta_hat, &p.delta, p.gene_phi.data()));
    return p;
}
// one result per test: labels per cell (-1 = in no group); mode 0 each group against the rest, mode 1 group 0 against group 1,
// mode 2 each group 1 .. n_groups - 1 against group 0 (a shared control); backend: the exact test's kernel (diff_exp.rs:125-161)
inline std::vector<DiffExpResult> sseq_de(const AdaptiveMat &m, const std::vector<int16_t> &labels, uint32_t n_groups, int mode,
                                          const SSeqParams &p, uint64_t big_count = BIG_COUNT_DEFAULT, Snoop *snoop = nullptr,
                                          NbExactBackend backend = NbExactBackend::LogSpace) {
    const uint64_t g = m.rows();
    const uint32_t t = mode == 0 ? n_groups : mode == 2 && n_groups > 0 ? n_groups - 1 : 1;
    std::vector<uint64_t> si(g * t), so(g * t);
    std::vector<double> pv(g * t), pa(g * t), l2(g * t), mi(g * t), mo(g * t);
    scanrs_snoop sn = detail::make_snoop(snoop);
    check(scanrs_sseq_de_backend(m.raw(), labels.data(), n_groups, mode, p.size_factors.data(), p.gene_means.data(), p.gene_phi.data(),
                                 p.use_genes.data(), big_count, (int)backend, snoop ? &sn : nullptr, si.data(), so.data(), pv.data(), pa.data(),
                                 l2.data(), mi.data(), mo.data()));
    std::vector<DiffExpResult> out(t);
    for (uint32_t j = 0; j < t; j++) {
        DiffExpResult &r = out[j];
        for (uint64_t i = 0; i < g; i++) {
            const uint64_t o = i * t + j;
            r.sums_in.push_back(si[o]);
            r.sums_out.push_back(so[o]);
            r.p_values.push_back(pv[o]);
            r.adjusted_p_values.push_back(pa[o]);
            r.log2_fold_change.push_back(l2[o]);
            r.normalized_mean_in.push_back(mi[o]);
            r.normalized_mean_out.push_back(mo[o]);
        }
    }
    return out;
}
// The same two calls over the shards of a MultiMat (scanrs_multi_sseq_params, scanrs_multi_sseq_de): the cells must be the sharded
// dimension - a genes x cells CSC matrix, or a cells x genes CSR one with transposed = true. Arguments and results span the whole
// matrix and equal those of an unsharded handle bit for bit.
inline SSeqParams compute_sseq_params(const MultiMat &m, bool transposed = false, double zeta_quintile = ZETA_QUINTILE_DEFAULT,
                                      const std::vector<uint64_t> *cell_indices = nullptr, const std::vector<double> *umi_counts = nullptr) {
    SSeqParams p;
    const uint64_t g = transposed ? m.cols() : m.rows(), c = transposed ? m.rows() : m.cols();
    p.num_genes = (uint32_t)g;
    p.num_cells = (uint32_t)(cell_indices ? cell_indices->size() : c);
    p.size_factors.resize(c);
    p.gene_means.resize(g);
    p.gene_variances.resize(g);
    p.use_genes.resize(g);
    p.gene_moment_phi.resize(g);
    p.gene_phi.resize(g);
    check(scanrs_multi_sseq_params(m.raw(), transposed ? 1 : 0, zeta_quintile, cell_indices ? cell_indices->data() : nullptr,
                                   cell_indices ? cell_indices->size() : 0, umi_counts ? umi_counts->data() : nullptr, p.size_factors.data(),
                                   p.gene_means.data(), p.gene_variances.data(), p.use_genes.data(), p.gene_moment_phi.data(), &p.zeta_hat, &p.delta,
                                   p.gene_phi.data()));
    return p;
}
inline std::vector<uint64_t> group_sums(const MultiMat &m, bool transposed, const std::vector<int16_t> &labels, uint32_t n_groups) {
    std::vector<uint64_t> sums((transposed ? m.cols() : m.rows()) * n_groups);
    check(scanrs_multi_group_sums(m.raw(), transposed ? 1 : 0, labels.data(), n_groups, sums.data(), nullptr));
    return sums;
}
inline std::vector<DiffExpResult> sseq_de(const MultiMat &m, bool transposed, const std::vector<int16_t> &labels, uint32_t n_groups, int mode,
                                          const SSeqParams &p, uint64_t big_count = BIG_COUNT_DEFAULT, Snoop *snoop = nullptr,
                                          NbExactBackend backend = NbExactBackend::LogSpace) {
    const uint64_t g = transposed ? m.cols() : m.rows();
    const uint32_t t = mode == 0 ? n_groups : mode == 2 && n_groups > 0 ? n_groups - 1 : 1;
    std::vector<uint64_t> si(g * t), so(g * t);
    std::vector<double> pv(g * t), pa(g * t), l2(g * t), mi(g * t), mo(g * t);
    scanrs_snoop sn = detail::make_snoop(snoop);
    check(scanrs_multi_sseq_de(m.raw(), transposed ? 1 : 0, labels.data(), n_groups, mode, p.size_factors.data(), p.gene_means.data(),
                               p.gene_phi.data(), p.use_genes.data(), big_count, (int)backend, snoop ? &sn : nullptr, si.data(), so.data(), pv.data(),
                               pa.data(), l2.data(), mi.data(), mo.data()));
    std::vector<DiffExpResult> out(t);
    for (uint32_t j = 0; j < t; j++) {
        DiffExpResult &r = out[j];
        for (uint64_t i = 0; i < g; i++) {
            const uint64_t o = i * t + j;
            r.sums_in.push_back(si[o]);
            r.sums_out.push_back(so[o]);
            r.p_values.push_back(pv[o]);
            r.adjusted_p_values.push_back(pa[o]);
            r.log2_fold_change.push_back(l2[o]);
            r.normalized_mean_in.push_back(mi[o]);
            r.normalized_mean_out.push_back(mo[o]);
        }
    }
    return out;
}
// sseq_de_from_sums (diff_exp.rs:177-198) for one test: per-gene sums of the two sides and their size factors
inline DiffExpResult sseq_de_from_sums(const std::vector<uint64_t> &sums_a, const std::vector<uint64_t> &sums_b, double size_factor_a,
                                       double size_factor_b, const SSeqParams &p, NbExactBackend backend = NbExactBackend::LogSpace,
                                       uint64_t big_count = BIG_COUNT_DEFAULT, Snoop *snoop = nullptr) {
    const uint64_t g = sums_a.size();
    DiffExpResult r;
    r.sums_in = sums_a;
    r.sums_out = sums_b;
    for (auto *v : {&r.p_values, &r.adjusted_p_values, &r.log2_fold_change, &r.normalized_mean_in, &r.normalized_mean_out}) v->resize(g);
    scanrs_snoop sn = detail::make_snoop(snoop);
    check(scanrs_sseq_de_from_sums_backend(g, 1, sums_a.data(), sums_b.data(), &size_factor_a, &size_factor_b, p.gene_means.data(),
                                           p.gene_phi.data(), p.use_genes.data(), big_count, (int)backend, snoop ? &sn : nullptr, r.p_values.data(),
                                           r.adjusted_p_values.data(), r.log2_fold_change.data(), r.normalized_mean_in.data(),
                                           r.normalized_mean_out.data()));
    return r;
}
// scanrs_sseq_de_pairs: test j is compute_sseq_params over the union of groups pairs[j].first and .second (diff_exp.rs:458-490), then
// the first group against the second (diff_exp.rs:125-161): merge_clusters.rs' candidates, batched (see diff_exp.rs:361-376)
struct PairParams : SSeqParams { // size_factors stays empty, as in sseq_params_from_moments
    double size_factor_a = 0.0, size_factor_b = 0.0, median_total = 0.0, sum_size_factors = 0.0;
    uint64_t num_cells_a = 0, num_cells_b = 0;
    bool literal = false; // the union's median total was 0: the pair ran the two reference calls themselves
};
// `call` is one of the three entry points with the handle bound: (labels, n_groups, pair_a, pair_b, n_pairs, ..., params) -> code
template <typename Call>
inline std::pair<std::vector<DiffExpResult>, std::vector<PairParams>> sseq_de_pairs_with(
    Call &&call, uint64_t g, const std::vector<int16_t> &labels, uint32_t n_groups, const std::vector<std::pair<uint32_t, uint32_t>> &pairs,
    double zeta_quintile, uint64_t big_count, NbExactBackend backend, Snoop *snoop) {
    const uint32_t t = (uint32_t)pairs.size();
    std::vector<uint32_t> pa(t), pb(t);
    for (uint32_t j = 0; j < t; j++) pa[j] = pairs[j].first, pb[j] = pairs[j].second;
    std::vector<uint64_t> si(g * t), so(g * t), na(t), nb(t);
    std::vector<double> pv(g * t), pq(g * t), l2(g * t), mi(g * t), mo(g * t), mean(g * t), var(g * t), mm(g * t), phi(g * t);
    std::vector<double> zh(t), dl(t), fa(t), fb(t), med(t), ssf(t);
    std::vector<uint8_t> use(g * t), lit(t);
    scanrs_sseq_pair_params pp = {mean.data(), var.data(), mm.data(), phi.data(), use.data(), zh.data(), dl.data(), fa.data(),
                                  fb.data(), med.data(), ssf.data(), na.data(), nb.data(), lit.data()};
    scanrs_snoop sn = detail::make_snoop(snoop);
    check(call(labels.data(), n_groups, pa.data(), pb.data(), t, zeta_quintile, big_count, (int)backend, snoop ? &sn : nullptr, si.data(), so.data(),
               pv.data(), pq.data(), l2.data(), mi.data(), mo.data(), &pp));
    std::vector<DiffExpResult> out(t);
    std::vector<PairParams> prm(t);
    for (uint32_t j = 0; j < t; j++) {
        DiffExpResult &r = out[j];
        PairParams &q = prm[j];
        q.num_genes = (uint32_t)g;
        q.num_cells = (uint32_t)(na[j] + nb[j]);
        q.zeta_hat = zh[j], q.delta = dl[j], q.size_factor_a = fa[j], q.size_factor_b = fb[j], q.median_total = med[j];
        q.sum_size_factors = ssf[j], q.num_cells_a = na[j], q.num_cells_b = nb[j], q.literal = lit[j] != 0;
        for (uint64_t i = 0; i < g; i++) {
            const uint64_t o = i * t + j;
            r.sums_in.push_back(si[o]);
            r.sums_out.push_back(so[o]);
            r.p_values.push_back(pv[o]);
            r.adjusted_p_values.push_back(pq[o]);
            r.log2_fold_change.push_back(l2[o]);
            r.normalized_mean_in.push_back(mi[o]);
            r.normalized_mean_out.push_back(mo[o]);
            q.gene_means.push_back(mean[o]);
            q.gene_variances.push_back(var[o]);
            q.use_genes.push_back(use[o]);
            q.gene_moment_phi.push_back(mm[o]);
            q.gene_phi.push_back(phi[o]);
        }
    }
    return {std::move(out), std::move(prm)};
}
inline std::pair<std::vector<DiffExpResult>, std::vector<PairParams>> sseq_de_pairs(
    const AdaptiveMat &m, const std::vector<int16_t> &labels, uint32_t n_groups, const std::vector<std::pair<uint32_t, uint32_t>> &pairs,
    double zeta_quintile = ZETA_QUINTILE_DEFAULT, uint64_t big_count = BIG_COUNT_DEFAULT, NbExactBackend backend = NbExactBackend::LogSpace,
    Snoop *snoop = nullptr) {
    return sseq_de_pairs_with([&](auto... a) { return scanrs_sseq_de_pairs(m.raw(), a...); }, m.rows(), labels, n_groups, pairs, zeta_quintile,
                              big_count, backend, snoop);
}
// The collective form on one sharded handle (every rank calls it with the same arguments; labels span the whole matrix), and the same
// over the shards of a MultiMat from one process (scanrs_sseq_de_pairs_sharded, scanrs_multi_sseq_de_pairs): the cells
// must be the sharded dimension, and every output equals the unsharded call's bit for bit.
inline std::pair<std::vector<DiffExpResult>, std::vector<PairParams>> sseq_de_pairs_sharded(
    const AdaptiveMat &m, const std::vector<int16_t> &labels, uint32_t n_groups, const std::vector<std::pair<uint32_t, uint32_t>> &pairs,
    double zeta_quintile = ZETA_QUINTILE_DEFAULT, uint64_t big_count = BIG_COUNT_DEFAULT, NbExactBackend backend = NbExactBackend::LogSpace,
    Snoop *snoop = nullptr) {
    return sseq_de_pairs_with([&](auto... a) { return scanrs_sseq_de_pairs_sharded(m.raw(), a...); }, m.rows(), labels, n_groups, pairs,
                              zeta_quintile, big_count, backend, snoop);
}
inline std::pair<std::vector<DiffExpResult>, std::vector<PairParams>> sseq_de_pairs(
    const MultiMat &m, bool transposed, const std::vector<int16_t> &labels, uint32_t n_groups,
    const std::vector<std::pair<uint32_t, uint32_t>> &pairs, double zeta_quintile = ZETA_QUINTILE_DEFAULT, uint64_t big_count = BIG_COUNT_DEFAULT,
    NbExactBackend backend = NbExactBackend::LogSpace, Snoop *snoop = nullptr) {
    return sseq_de_pairs_with([&](auto... a) { return scanrs_multi_sseq_de_pairs(m.raw(), transposed ? 1 : 0, a...); },
                              transposed ? m.cols() : m.rows(), labels, n_groups, pairs, zeta_quintile, big_count, backend, snoop);
}
// percentile_of_sorted(.., 50) (stat.rs:140-162) of the union of two ascending lists, on the host
inline double host_union_median(const std::vector<double> &a, const std::vector<double> &b) {
    double out = 0.0;
    check(scanrs_host_union_median(a.data(), a.size(), b.data(), b.size(), &out));
    return out;
}
// nb_exact_test_ratio (dist.rs:155-215) and nb_exact_ratio_step (dist.rs:124-126) on the host
inline double host_nb_exact_test_ratio(uint64_t x_a, uint64_t x_b, double sf_a, double sf_b, double mu, double phi) {
    double p = 0.0;
    check(scanrs_host_nb_exact_test_ratio(x_a, x_b, sf_a, sf_b, mu, phi, &p));
    return p;
}
inline double host_nb_exact_ratio_step(double k, double n, double sa_r, double sb_r) {
    double out = 0.0;
    check(scanrs_host_nb_exact_ratio_step(k, n, sa_r, sb_r, &out));
    return out;
}
inline std::vector<uint64_t> group_sums(const AdaptiveMat &m, const std::vector<int16_t> &labels, uint32_t n_groups) { // genes x n_groups
    std::vector<uint64_t> s(m.rows() * n_groups);
    check(scanrs_mat_group_sums(m.raw(), labels.data(), n_groups, s.data(), nullptr));
    return s;
}
} // namespace diff_exp

namespace cluster {
// merge_clusters (scan-rs/src/merge_clusters.rs), linkage.rs, median_mut (stats.rs): labels 0 .. K-1, every value present
inline std::vector<double> pdist(const std::vector<double> &x, uint64_t m, uint32_t d) { // linkage.rs:14-26
    std::vector<double> out(m > 1 ? m * (m - 1) / 2 : 0);
    check(scanrs_host_pdist(x.data(), m, d, out.data()));
    return out;
}
inline std::vector<double> linkage(const std::vector<double> &x, uint64_t m, uint32_t d) { // Complete: (m - 1) x 4, linkage.rs:43-158
    std::vector<double> z(m > 1 ? (m - 1) * 4 : 0);
    check(scanrs_host_linkage_complete(x.data(), m, d, z.data()));
    return z;
}
inline std::vector<int16_t> relabel_by_size(const std::vector<int16_t> &labels) { // merge_clusters.rs:43-56
    std::vector<int16_t> out(labels.size());
    check(scanrs_host_relabel_by_size(labels.data(), labels.size(), out.data()));
    return out;
}
// merge_clusters.rs:20-40: k x d medians; pca n x d with leading dimension ld (host array)
inline std::vector<double> medioids(const double *pca, uint64_t n, uint32_t ld, uint32_t d, const std::vector<int16_t> &labels, uint32_t k) {
    std::vector<double> out((size_t)k * d);
    check(scanrs_cluster_medoids(pca, n, ld, d, labels.data(), k, out.data()));
    return out;
}
inline std::vector<double> medioids_device(const double *d_pca, uint64_t n, uint32_t ld, uint32_t d, const std::vector<int16_t> &labels,
                                           uint32_t k) {
    std::vector<double> out((size_t)k * d);
    check(scanrs_cluster_medoids_device(d_pca, n, ld, d, labels.data(), k, out.data()));
    return out;
}
struct MergeCandidate {
    int16_t leaf0, leaf1;
    uint64_t n_de;
    double min_p_adj;
};
struct MergeTrace {
    std::vector<MergeCandidate> candidates;
    uint64_t n_candidates = 0, n_rounds = 0, n_merges = 0, n_passes = 0;
};
// `call` is one of the three entry points with the handle and the scores bound: (labels, labels_out, snoop, trace) -> code
template <typename Call>
inline std::vector<int16_t> merge_clusters_with(Call &&call, const std::vector<int16_t> &labels, MergeTrace *trace, Snoop *snoop, uint64_t capacity) {
    std::vector<int16_t> out(labels.size());
    scanrs_snoop sn = detail::make_snoop(snoop);
    std::vector<int16_t> l0(capacity), l1(capacity);
    std::vector<uint64_t> nde(capacity);
    std::vector<double> mp(capacity);
    scanrs_merge_trace t{capacity, l0.data(), l1.data(), nde.data(), mp.data(), 0, 0, 0, 0};
    check(call(labels.data(), out.data(), snoop ? &sn : nullptr, trace ? &t : nullptr));
    if (trace) {
        trace->candidates.clear();
        for (uint64_t i = 0; i < t.n_candidates && i < capacity; i++) trace->candidates.push_back({l0[i], l1[i], nde[i], mp[i]});
        trace->n_candidates = t.n_candidates;
        trace->n_rounds = t.n_rounds;
        trace->n_merges = t.n_merges;
        trace->n_passes = t.n_passes;
    }
    return out;
}
// merge_clusters.rs:59-138: pca is cells x d (leading dimension ld), in device memory when pca_is_device
inline std::vector<int16_t> merge_clusters(const AdaptiveMat &m, const double *pca, bool pca_is_device, uint32_t ld, uint32_t d,
                                           const std::vector<int16_t> &labels, MergeTrace *trace = nullptr, Snoop *snoop = nullptr,
                                           uint64_t capacity = 4096) {
    return merge_clusters_with([&](auto... a) { return scanrs_merge_clusters(m.raw(), pca, pca_is_device ? 1 : 0, ld, d, a...); }, labels, trace,
                               snoop, capacity);
}
// The collective forms on one sharded handle (every rank calls them with the same arguments; labels span the whole matrix, and so does a
// host pca; a device pca holds the rank's own cells), and the same over the shards of a MultiMat from one process (pca: a host array
// over all cells). The cells must be the sharded dimension; results equal the unsharded call's bit for bit.
inline std::vector<int16_t> merge_clusters_sharded(const AdaptiveMat &m, const double *pca, bool pca_is_device, uint32_t ld, uint32_t d,
                                                   const std::vector<int16_t> &labels, MergeTrace *trace = nullptr, Snoop *snoop = nullptr,
                                                   uint64_t capacity = 4096) {
    return merge_clusters_with([&](auto... a) { return scanrs_merge_clusters_sharded(m.raw(), pca, pca_is_device ? 1 : 0, ld, d, a...); }, labels,
                               trace, snoop, capacity);
}
inline std::vector<int16_t> merge_clusters(const MultiMat &m, bool transposed, const double *pca, uint32_t ld, uint32_t d,
                                           const std::vector<int16_t> &labels, MergeTrace *trace = nullptr, Snoop *snoop = nullptr,
                                           uint64_t capacity = 4096) {
    return merge_clusters_with([&](auto... a) { return scanrs_multi_merge_clusters(m.raw(), transposed ? 1 : 0, pca, ld, d, a...); }, labels, trace,
                               snoop, capacity);
}
inline std::vector<double> cluster_medoids_sharded(const AdaptiveMat &m, const double *pca, bool pca_is_device, uint32_t ld, uint32_t d,
                                                   const std::vector<int16_t> &labels, uint32_t k) {
    std::vector<double> out((size_t)k * d);
    check(scanrs_cluster_medoids_sharded(m.raw(), pca, pca_is_device ? 1 : 0, ld, d, labels.data(), k, out.data()));
    return out;
}
inline std::vector<double> cluster_medoids(const MultiMat &m, bool transposed, const double *pca, uint32_t ld, uint32_t d,
                                           const std::vector<int16_t> &labels, uint32_t k) {
    std::vector<double> out((size_t)k * d);
    check(scanrs_multi_cluster_medoids(m.raw(), transposed ? 1 : 0, pca, ld, d, labels.data(), k, out.data()));
    return out;
}
} // namespace cluster

// hclust/src/lib.rs: HierarchicalCluster over a Euclidean dendrogram made on the device
namespace hclust {
enum class LinkageMethod : int { Single = 0, Complete = 1, Average = 2, Weighted = 3, Ward = 4, Centroid = 5, Median = 6 }; // kodama::Method
enum class ClusterDirection : int { Rows = 0, Columns = 1 };                                                              // :30-35
enum class LeafOrdering : int { Naive = 0, ModularSmallest = 1 };                                                         // :53-59

struct Steps { // kodama::Dendrogram's steps, n - 1 entries each
    std::vector<uint32_t> cluster1, cluster2, size;
    std::vector<double> dissimilarity;
};

class HierarchicalCluster {
    scanrs_hclust *h_ = nullptr;
    explicit HierarchicalCluster(scanrs_hclust *h) : h_(h) {}

  public:
    // HierarchicalCluster::new (:132-148): x is rows x cols, leading dimension ld, in host memory or (x_is_device) in device memory
    HierarchicalCluster(const double *x, bool x_is_device, uint64_t rows, uint64_t cols, uint64_t ld, LinkageMethod method, ClusterDirection direction,
                        Snoop *snoop = nullptr) {
        scanrs_snoop sn = detail::make_snoop(snoop);
        check((x_is_device ? scanrs_hclust_create_device : scanrs_hclust_create)(x, rows, cols, ld, (int)direction, (int)method, snoop ? &sn : nullptr, &h_));
    }
    HierarchicalCluster(const Array2 &a, LinkageMethod method, ClusterDirection direction, Snoop *snoop = nullptr)
        : HierarchicalCluster(a.data.data(), false, a.rows, a.cols, a.cols, method, direction, snoop) {}
    static HierarchicalCluster from_steps(const Steps &s) { // a given, already sorted dendrogram (host only)
        scanrs_hclust *h = nullptr;
        check(scanrs_hclust_from_steps(s.cluster1.size() + 1, s.cluster1.data(), s.cluster2.data(), s.dissimilarity.data(), s.size.data(), &h));
        return HierarchicalCluster(h);
    }
    HierarchicalCluster(const HierarchicalCluster &) = delete;
    HierarchicalCluster &operator=(const HierarchicalCluster &) = delete;
    HierarchicalCluster(HierarchicalCluster &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    HierarchicalCluster &operator=(HierarchicalCluster &&o) noexcept {
        if (this != &o) {
            scanrs_hclust_free(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~HierarchicalCluster() { scanrs_hclust_free(h_); }
    scanrs_hclust *raw() const { return h_; }
    uint64_t observations() const {
        uint64_t n = 0;
        check(scanrs_hclust_n(h_, &n));
        return n;
    }
    Steps steps() const {
        const uint64_t m = observations() - 1;
        Steps s{std::vector<uint32_t>(m), std::vector<uint32_t>(m), std::vector<uint32_t>(m), std::vector<double>(m)};
        check(scanrs_hclust_steps(h_, s.cluster1.data(), s.cluster2.data(), s.dissimilarity.data(), s.size.data()));
        return s;
    }
    std::vector<uint32_t> leaves(LeafOrdering ordering) const { // :201-206
        std::vector<uint32_t> out(observations());
        check(scanrs_hclust_leaves(h_, (int)ordering, out.data()));
        return out;
    }
    std::vector<uint32_t> merge_clusters_below_distance_threshold(double threshold) const { // :210-227
        std::vector<uint32_t> out(observations());
        check(scanrs_hclust_merge_below(h_, threshold, out.data()));
        return out;
    }
    std::vector<uint32_t> fcluster(uint64_t num_clusters) const { // :231-239
        std::vector<uint32_t> out(observations());
        check(scanrs_hclust_fcluster(h_, num_clusters, out.data()));
        return out;
    }
    // chain steps, launches, batches, bytes of the matrix, microseconds of the distance pass and of the chain, merges
    std::array<uint64_t, 7> info() const {
        std::array<uint64_t, 7> out{};
        check(scanrs_hclust_info(h_, out.data(), 7));
        return out;
    }
};
// the host twin of the device chain (tests and small inputs): x is n x d compact
inline Steps host_linkage(const std::vector<double> &x, uint64_t n, uint32_t d, LinkageMethod method) {
    const uint64_t m = n ? n - 1 : 0;
    Steps s{std::vector<uint32_t>(m), std::vector<uint32_t>(m), std::vector<uint32_t>(m), std::vector<double>(m)};
    check(scanrs_host_hclust_linkage(x.data(), n, d, (int)method, s.cluster1.data(), s.cluster2.data(), s.dissimilarity.data(), s.size.data()));
    return s;
}
inline std::vector<double> debug_pdist(const std::vector<double> &x, uint64_t n, uint32_t d, uint64_t ld, bool squared) {
    std::vector<double> out(n ? n * (n - 1) / 2 : 0);
    check(scanrs_debug_hclust_pdist(x.data(), n, d, ld, squared ? 1 : 0, out.data()));
    return out;
}
} // namespace hclust

// nn::knn (nn.rs:38-83) where the scores stay sharded: global indices, equal to `knn` of the whole point set bit for bit
struct KnnResult {
    std::vector<uint32_t> indices; // rows x k, nearest first, UINT32_MAX padded
    std::vector<double> sq_dist;   // rows x k when asked for, +inf in padded slots
};
// COLLECTIVE on one sharded handle: points is a host array over all cells, or the rank's own n_local rows in device memory
inline KnnResult knn_sharded(const AdaptiveMat &m, uint64_t n_local, const double *points, bool points_is_device, uint32_t ld, uint32_t d, size_t k,
                             bool with_sq_dist = false) {
    KnnResult r;
    r.indices.assign((size_t)n_local * k, 0u);
    if (with_sq_dist) r.sq_dist.assign((size_t)n_local * k, 0.0);
    check(scanrs_knn_sharded(m.raw(), points, points_is_device ? 1 : 0, ld, d, (uint32_t)k, r.indices.data(), with_sq_dist ? r.sq_dist.data() : nullptr));
    return r;
}
// over the shards of a MultiMat from one process; points == nullptr: the scores its last run_pca left on the devices
inline KnnResult knn(const MultiMat &m, uint64_t cells, const double *points, uint32_t ld, uint32_t d, size_t k, bool with_sq_dist = false) {
    KnnResult r;
    r.indices.assign((size_t)cells * k, 0u);
    if (with_sq_dist) r.sq_dist.assign((size_t)cells * k, 0.0);
    check(scanrs_multi_knn(m.raw(), points, ld, d, (uint32_t)k, r.indices.data(), with_sq_dist ? r.sq_dist.data() : nullptr));
    return r;
}
// the merge rule of that search on the host: two sorted, padded lists of k entries that share no index -> the first k of their union
inline void host_knn_merge(uint32_t k, const double *da, const uint32_t *ia, const double *db, const uint32_t *ib, double *dout, uint32_t *iout) {
    check(scanrs_host_knn_merge(k, da, ia, db, ib, dout, iout));
}
// umap_rs::knn::nearest_neighbors (umap-rs/src/knn.rs:112-166) under `DistanceType` (dist.rs:12-35): indices and distances of the k
// nearest other rows, n x min(k, n - 1) each as the reference returns them (the euclidean kind is the library's search)
enum class DistanceType : int { Euclidean = SCANRS_DIST_EUCLIDEAN, Pearson = SCANRS_DIST_PEARSON, Cosine = SCANRS_DIST_COSINE };
struct NearestNeighbors {
    size_t k = 0;                  // min(k, n - 1)
    std::vector<uint32_t> indices; // n x k, nearest first
    std::vector<double> distances; // n x k
};
namespace detail {
template <typename F>
inline NearestNeighbors nearest_neighbors_call(size_t n, size_t k, F &&call) {
    std::vector<uint32_t> idx(n * k);
    std::vector<double> dist(n * k);
    check(call(idx.data(), dist.data()));
    NearestNeighbors r;
    r.k = n ? (k < n - 1 ? k : n - 1) : 0;
    r.indices.resize(n * r.k);
    r.distances.resize(n * r.k);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < r.k; j++) r.indices[i * r.k + j] = idx[i * k + j], r.distances[i * r.k + j] = dist[i * k + j];
    return r;
}
} // namespace detail
inline NearestNeighbors nearest_neighbors(const Array2 &data, size_t k, DistanceType distance_type) {
    return detail::nearest_neighbors_call(data.rows, k, [&](uint32_t *i, double *d) {
        return scanrs_nearest_neighbors(data.data.data(), data.rows, (uint32_t)data.cols, (uint32_t)k, (int)distance_type, i, d);
    });
}
// on points that are already in device memory (e.g. PcaResultDevice d_v / ld_v)
inline NearestNeighbors nearest_neighbors_device(const double *d_data, size_t n, uint32_t ld, uint32_t d, size_t k, DistanceType distance_type) {
    return detail::nearest_neighbors_call(n, k, [&](uint32_t *i, double *dd) {
        return scanrs_nearest_neighbors_device(d_data, n, ld, d, (uint32_t)k, (int)distance_type, i, dd);
    });
}
// the host twin: the same answer by exhaustive search on the host, and the pieces the tests of the filtered route read
inline NearestNeighbors host_nearest_neighbors(const Array2 &data, size_t k, DistanceType distance_type) {
    return detail::nearest_neighbors_call(data.rows, k, [&](uint32_t *i, double *d) {
        return scanrs_host_nearest_neighbors(data.data.data(), data.rows, (uint32_t)data.cols, (uint32_t)k, (int)distance_type, i, d);
    });
}
// A query set of its own: indices into `points`, n_q x min(k, n_p), padded with UINT32_MAX / +inf where a row has
// fewer admissible points; include_self == false drops the point whose index equals the query's row number.
namespace detail {
template <typename F>
inline NearestNeighbors nearest_neighbors_query_call(size_t n_q, size_t n_p, size_t k, F &&call) {
    std::vector<uint32_t> idx(n_q * k);
    std::vector<double> dist(n_q * k);
    check(call(idx.data(), dist.data()));
    NearestNeighbors r;
    r.k = k < n_p ? k : n_p;
    r.indices.resize(n_q * r.k);
    r.distances.resize(n_q * r.k);
    for (size_t i = 0; i < n_q; i++)
        for (size_t j = 0; j < r.k; j++) r.indices[i * r.k + j] = idx[i * k + j], r.distances[i * r.k + j] = dist[i * k + j];
    return r;
}
} // namespace detail
inline NearestNeighbors nearest_neighbors_query(const Array2 &queries, const Array2 &points, size_t k, DistanceType distance_type,
                                                bool include_self = true) {
    if (queries.cols != points.cols) throw std::invalid_argument("Dimension mismatch");
    return detail::nearest_neighbors_query_call(queries.rows, points.rows, k, [&](uint32_t *i, double *d) {
        return scanrs_nearest_neighbors_query(queries.data.data(), queries.rows, points.data.data(), points.rows, (uint32_t)points.cols, (uint32_t)k,
                                              (int)distance_type, include_self ? 1 : 0, i, d);
    });
}
inline NearestNeighbors nearest_neighbors_query_device(const double *d_queries, size_t n_q, uint32_t ld_q, const double *d_points, size_t n_p,
                                                       uint32_t ld_p, uint32_t d, size_t k, DistanceType distance_type, bool include_self = true) {
    return detail::nearest_neighbors_query_call(n_q, n_p, k, [&](uint32_t *i, double *dd) {
        return scanrs_nearest_neighbors_query_device(d_queries, n_q, ld_q, d_points, n_p, ld_p, d, (uint32_t)k, (int)distance_type,
                                                     include_self ? 1 : 0, i, dd);
    });
}
inline NearestNeighbors host_nearest_neighbors_query(const Array2 &queries, const Array2 &points, size_t k, DistanceType distance_type,
                                                     bool include_self = true) {
    if (queries.cols != points.cols) throw std::invalid_argument("Dimension mismatch");
    return detail::nearest_neighbors_query_call(queries.rows, points.rows, k, [&](uint32_t *i, double *d) {
        return scanrs_host_nearest_neighbors_query(queries.data.data(), queries.rows, points.data.data(), points.rows, (uint32_t)points.cols,
                                                   (uint32_t)k, (int)distance_type, include_self ? 1 : 0, i, d);
    });
}
// Where the points stay sharded: GLOBAL indices, equal to nearest_neighbors of the whole point set in every bit.
// COLLECTIVE on one sharded handle; the result is n_local x k, padded with UINT32_MAX / +inf from column min(k, n - 1) on
inline NearestNeighbors nearest_neighbors_sharded(const AdaptiveMat &m, uint64_t n_local, const double *points, bool points_is_device, uint32_t ld,
                                                  uint32_t d, size_t k, DistanceType distance_type) {
    NearestNeighbors r;
    r.k = k;
    r.indices.assign((size_t)n_local * k, 0xFFFFFFFFu);
    r.distances.assign((size_t)n_local * k, std::numeric_limits<double>::infinity());
    check(scanrs_nearest_neighbors_sharded(m.raw(), points, points_is_device ? 1 : 0, ld, d, (uint32_t)k, (int)distance_type, r.indices.data(),
                                           r.distances.data()));
    return r;
}
// over the shards of a MultiMat from one process; points == nullptr: the scores its last run_pca left on the devices
inline NearestNeighbors nearest_neighbors(const MultiMat &m, uint64_t cells, const double *points, uint32_t ld, uint32_t d, size_t k,
                                          DistanceType distance_type) {
    return detail::nearest_neighbors_call(cells, k, [&](uint32_t *i, double *dd) {
        return scanrs_multi_nearest_neighbors(m.raw(), points, ld, d, (uint32_t)k, (int)distance_type, i, dd);
    });
}
inline void host_distance(DistanceType distance_type, const double *x, const double *y, uint32_t d, double *key, double *dist) {
    check(scanrs_host_distance((int)distance_type, x, y, d, key, dist));
}
inline void host_metric_rows(DistanceType distance_type, const double *data, uint64_t n, uint32_t d, double *c, double *s, double *z) {
    check(scanrs_host_metric_rows((int)distance_type, data, n, d, c, s, z));
}
inline void debug_nearest_neighbors_params(double *delta, double *e, double *chain, double *sxx_min, double *sxx_max) {
    check(scanrs_debug_nearest_neighbors_params(delta, e, chain, sxx_min, sxx_max));
}

// umap_rs::fuzzy::fuzzy_simplicial_set (umap-rs/src/fuzzy.rs:30-62) and the pruned edge list of initialize_simplicial_set_embedding
// (embedding.rs:38-53, 75-85, without the shuffle); DESIGN.md §7r. The defaults are the ones umap.rs passes.
struct FuzzyParams {
    double local_connectivity = 1.0, set_op_mix_ratio = 1.0;
    bool apply_fuzzy_combine = true;
    uint32_t n_iter = 0;    // 0 = the reference's 64
    double bandwidth = 0.0; // 0.0 = the reference's 1.0
    scanrs_fuzzy_params raw() const { return scanrs_fuzzy_params{local_connectivity, set_op_mix_ratio, apply_fuzzy_combine ? 1 : 0, n_iter, bandwidth}; }
};
struct GraphEdges {
    std::vector<uint32_t> head, tail;
    std::vector<double> weights, epochs_per_sample;
};
struct CsrGraph {
    std::vector<uint64_t> indptr;
    std::vector<uint32_t> indices;
    std::vector<double> values;
};
class FuzzyGraph {
    scanrs_graph *h_ = nullptr;
    explicit FuzzyGraph(scanrs_graph *h) : h_(h) {}

  public:
    // fuzzy_simplicial_set of host lists (n x k); host_only: the twin (scanrs_host_fuzzy_simplicial_set), no device
    FuzzyGraph(const uint32_t *knn_indices, const double *knn_distances, uint64_t n, uint32_t k, const FuzzyParams &p = FuzzyParams(),
               bool host_only = false) {
        const scanrs_fuzzy_params r = p.raw();
        check((host_only ? scanrs_host_fuzzy_simplicial_set : scanrs_fuzzy_simplicial_set)(knn_indices, knn_distances, n, k, &r, &h_));
    }
    // the lists already in device memory, leading dimension ld >= k
    static FuzzyGraph from_device_lists(const uint32_t *d_knn_indices, const double *d_knn_distances, uint64_t n, uint32_t ld, uint32_t k,
                                        const FuzzyParams &p = FuzzyParams()) {
        const scanrs_fuzzy_params r = p.raw();
        scanrs_graph *h = nullptr;
        check(scanrs_fuzzy_simplicial_set_device(d_knn_indices, d_knn_distances, n, ld, k, &r, &h));
        return FuzzyGraph(h);
    }
    // nearest_neighbors and the graph in one go, the lists never leaving the device (umap.rs:89-100)
    static FuzzyGraph umap_graph(const Array2 &points, size_t k, DistanceType distance_type, const FuzzyParams &p = FuzzyParams()) {
        const scanrs_fuzzy_params r = p.raw();
        scanrs_graph *h = nullptr;
        check(scanrs_umap_graph(points.data.data(), points.rows, (uint32_t)points.cols, (uint32_t)k, (int)distance_type, &r, &h));
        return FuzzyGraph(h);
    }
    static FuzzyGraph umap_graph_device(const double *d_points, uint64_t n, uint32_t ld, uint32_t d, size_t k, DistanceType distance_type,
                                        const FuzzyParams &p = FuzzyParams()) {
        const scanrs_fuzzy_params r = p.raw();
        scanrs_graph *h = nullptr;
        check(scanrs_umap_graph_device(d_points, n, ld, d, (uint32_t)k, (int)distance_type, &r, &h));
        return FuzzyGraph(h);
    }
    FuzzyGraph(const FuzzyGraph &) = delete;
    FuzzyGraph &operator=(const FuzzyGraph &) = delete;
    FuzzyGraph(FuzzyGraph &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    FuzzyGraph &operator=(FuzzyGraph &&o) noexcept {
        if (this != &o) {
            scanrs_graph_free(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~FuzzyGraph() { scanrs_graph_free(h_); }
    scanrs_graph *raw() const { return h_; }
    uint64_t rows() const { return info(0); }
    uint64_t nnz() const { return info(1); }
    uint64_t info(uint32_t what) const { // 0: n, 1: nnz, 2: the width of the lists, 3: resident on the device
        uint64_t v[4] = {0, 0, 0, 0};
        check(scanrs_graph_info(h_, v, 4));
        return v[what & 3];
    }
    CsrGraph to_csr() const {
        CsrGraph g{std::vector<uint64_t>(rows() + 1), std::vector<uint32_t>(nnz()), std::vector<double>(nnz())};
        check(scanrs_graph_to_host(h_, g.indptr.data(), g.indices.data(), g.values.data()));
        return g;
    }
    void sigmas_rhos(std::vector<double> &sigmas, std::vector<double> &rhos) const {
        sigmas.assign(rows(), 0.0), rhos.assign(rows(), 0.0);
        check(scanrs_graph_sigmas_rhos(h_, sigmas.data(), rhos.data()));
    }
    void device(const uint64_t **d_indptr, const uint32_t **d_indices, const double **d_values) const {
        check(scanrs_graph_device(h_, d_indptr, d_indices, d_values));
    }
    GraphEdges edges(double n_epochs) const { // embedding.rs:38-53, 75-85: tail = row, head = column, in CSR order
        uint64_t m = 0;
        check(scanrs_graph_edge_count(h_, n_epochs, &m));
        GraphEdges e{std::vector<uint32_t>(m), std::vector<uint32_t>(m), std::vector<double>(m), std::vector<double>(m)};
        check(scanrs_graph_edges(h_, n_epochs, e.head.data(), e.tail.data(), e.weights.data(), e.epochs_per_sample.data()));
        return e;
    }
};
inline std::vector<double> host_fuzzy_exp(const std::vector<double> &x) {
    std::vector<double> out(x.size());
    check(scanrs_host_fuzzy_exp(x.data(), x.size(), out.data()));
    return out;
}
// smooth_knn_dist of one row (fuzzy.rs:117-145): sigma; *iterations = how many times psum was formed
inline double host_smooth_knn_dist(const std::vector<double> &distances, double rho, double bandwidth = 0.0, uint32_t n_iter = 0,
                                   uint32_t *iterations = nullptr) {
    double sigma = 0.0;
    check(scanrs_host_smooth_knn_dist(distances.data(), (uint32_t)distances.size(), rho, bandwidth, n_iter, &sigma, iterations));
    return sigma;
}
// compute_membership_strengths (fuzzy.rs:148-181): the COO triple; returns its length
inline uint64_t host_membership_strengths(const uint32_t *knn_indices, const double *knn_distances, uint64_t n, uint32_t k, const double *sigmas,
                                          const double *rhos, std::vector<uint32_t> &rows, std::vector<uint32_t> &cols, std::vector<double> &values) {
    rows.assign(n * k, 0), cols.assign(n * k, 0), values.assign(n * k, 0.0);
    uint64_t m = 0;
    check(scanrs_host_membership_strengths(knn_indices, knn_distances, n, k, sigmas, rhos, rows.data(), cols.data(), values.data(), &m));
    rows.resize(m), cols.resize(m), values.resize(m);
    return m;
}
// the plan of the fixed-point column moments (option "col_moments") on the host: accepted or not, and the two exponents
struct ColMomentsPlan {
    bool accept = false;
    int e1 = 0, e2 = 0;
};
inline ColMomentsPlan host_col_moments_plan(uint32_t max_count, const std::vector<int> &kinds, const std::vector<int> &on_summed_axis,
                                            const std::vector<double> &fmin_pos, const std::vector<double> &fmax, uint64_t n_outer, uint64_t n_inner,
                                            uint32_t n_wg, int mode) {
    if (on_summed_axis.size() != kinds.size() || fmin_pos.size() != kinds.size() || fmax.size() != kinds.size())
        throw Error(SCANRS_ERR_ARGUMENT, "host_col_moments_plan: one entry per link in every list");
    ColMomentsPlan p;
    int accept = 0;
    check(scanrs_host_col_moments_plan(max_count, (uint32_t)kinds.size(), kinds.data(), on_summed_axis.data(), fmin_pos.data(), fmax.data(), n_outer,
                                       n_inner, n_wg, mode, &accept, &p.e1, &p.e2));
    p.accept = accept != 0;
    return p;
}
// the projection plan of svd_bk on the host, from max |C| per column of Q (colmax.size() == b * n_iter)
struct BkPlan {
    bool reuse = false, last_direct = false, full_direct = false;
    uint64_t flagged_older = 0, limit_branch = 0, n_early = 0;
    double limit = 0.0, cmax_dense = 0.0;
    std::vector<uint32_t> direct;
};
inline BkPlan host_bk_plan(const std::vector<double> &colmax, uint32_t b, uint32_t n_iter, double reuse_cmax = 1e5, bool coef_valid = true) {
    BkPlan p;
    uint64_t out[7] = {};
    p.direct.assign(colmax.size() + 1, 0u);
    check(scanrs_host_bk_plan(colmax.data(), colmax.size(), b, n_iter, reuse_cmax, coef_valid ? 1 : 0, out, &p.limit, &p.cmax_dense, p.direct.data()));
    p.reuse = out[0] != 0, p.flagged_older = out[1], p.limit_branch = out[2], p.last_direct = out[4] != 0, p.full_direct = out[5] != 0, p.n_early = out[6];
    p.direct.resize((size_t)out[3]);
    return p;
}
// which sort the transposed copy of an n_outer x n_inner copy with the largest count max_value is built through (counter "transpose_route")
struct TransposePlan {
    int route = 0; // 1 packed 64-bit key, 2 pair sort
    uint32_t ib = 0, ob = 0, cb = 0;
};
inline TransposePlan host_transpose_plan(uint64_t n_outer, uint64_t n_inner, uint32_t max_value) {
    TransposePlan p;
    check(scanrs_host_transpose_plan(n_outer, n_inner, max_value, &p.route, &p.ib, &p.ob, &p.cb));
    return p;
}
// the tables of options (scope 0: of a handle, 1: of the process) and of counters, as the library holds them
struct OptionInfo {
    std::string name;
    double dflt = 0.0, lo = 0.0, hi = 0.0;
    bool open_lo = false, settable = false;
    uint32_t route_position = 0; // position + 1 in the options array of scanrs_host_spmm_route, 0: not in it
};
inline std::vector<OptionInfo> option_info(int scope) {
    std::vector<OptionInfo> all;
    const char *name = nullptr;
    OptionInfo o;
    uint32_t flags = 0;
    for (uint32_t i = 0; scanrs_host_option_info(scope, i, &name, &o.dflt, &o.lo, &o.hi, &flags) == SCANRS_OK; i++) {
        o.name = name, o.open_lo = (flags & SCANRS_OPTION_OPEN_LO) != 0, o.settable = (flags & SCANRS_OPTION_SETTABLE) != 0;
        o.route_position = flags >> SCANRS_OPTION_ROUTE_SHIFT;
        all.push_back(o);
    }
    return all;
}
// what the setter of that scope would store for `value` under `name`; throws where the setter refuses
inline double host_option_parse(int scope, const std::string &name, double value) {
    double stored = 0.0;
    check(scanrs_host_option_parse(scope, name.c_str(), value, &stored));
    return stored;
}
inline std::vector<std::string> counter_names() {
    std::vector<std::string> all;
    const char *name = nullptr;
    for (uint32_t i = 0; scanrs_host_counter_name(i, &name) == SCANRS_OK; i++) all.push_back(name);
    return all;
}

namespace mtx {
// scan_rs::mtx::load_mtx (scan-rs/src/mtx.rs:10-51): the CSR arrays; `.to_device()` is the AdaptiveMat the reference returns
inline hdf5_io::FeatureBarcodeMatrix read_mtx(const std::string &path) {
    scanrs_h5_matrix *h = nullptr;
    check(scanrs_mtx_read(path.c_str(), &h));
    return hdf5_io::detail::take(h);
}
inline AdaptiveMat load_mtx(const std::string &path) { return read_mtx(path).to_device(); }
} // namespace mtx

} // namespace scanrs
