// knn_metric.hpp — the arithmetic of nearest_neighbors under Pearson and cosine distance (umap-rs/src/dist.rs:69-124), one
// restatement for the kernels (knn_metric.hip) and the host twin (knn_metric_host.cpp). Both files are compiled with
// -ffp-contract=off: every operation below is a separate IEEE f64 operation, as in the reference (Rust does not contract).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KM_HD __host__ __device__
#else
#define KM_HD
#endif

namespace scanrs {
namespace knn_metric {

enum Kind { EUCLIDEAN = 0, PEARSON = 1, COSINE = 2 };

// The threshold of the filtered route, in the space of the standardised rows z (derivation: knn_metric.hip):
//   tau_z = 2 key_k^2 (1 + KM_DELTA) + KM_E;  KM_CHAIN of it is what the filter's own fma chain may add to the exact |z_q - z_p|^2
constexpr double KM_DELTA = 0x1p-40, KM_E = 0x1p-40, KM_CHAIN = 0x1p-44;
// the magnitude window of s_xx = |c|^2 over all rows: inside it no product s_xx s_yy, no square root and no quotient of the formula
// overflows or goes subnormal (2^-800 <= s_xx s_yy <= 2^800); a degenerate row (s_xx == 0) lies outside it
constexpr double KM_SXX_MIN = 0x1p-400, KM_SXX_MAX = 0x1p400;

// dist.rs:77-83 / 117-123. `f64::max(v, 0.0)`: a NaN operand loses, so NaN -> 0 (and so does every v <= 0)
KM_HD inline double pair_value(double s_xx, double s_yy, double s_xy) {
    if (s_xx == 0.0 && s_yy == 0.0) return 0.0;
    if (s_xy == 0.0) return 1.0;
    const double v = 1.0 - s_xy / sqrt(s_xx * s_yy);
    return v > 0.0 ? v : 0.0;
}

// What depends on one row only (dist.rs:74-76 / 107-115): c = x - mu (pearson) or x (cosine), s_xx = fold(acc + c_j c_j) from 0.0,
// and for the filter z = c / sqrt(s_xx) (all zero for a degenerate row). c and z have d entries; z may be null.
KM_HD inline double prepare_row(int kind, const double *x, uint32_t d, double *c, double *z) {
    double mu = 0.0;
    if (kind == PEARSON) {
        for (uint32_t j = 0; j < d; j++) mu = mu + x[j];
        mu = mu / (double)d;
    }
    double s = 0.0;
    for (uint32_t j = 0; j < d; j++) {
        const double cj = kind == PEARSON ? x[j] - mu : x[j];
        c[j] = cj;
        s = s + cj * cj; // powi(2) is c * c
    }
    if (z) {
        const double r = sqrt(s);
        for (uint32_t j = 0; j < d; j++) z[j] = s == 0.0 ? 0.0 : c[j] / r;
    }
    return s;
}

} // namespace knn_metric

// knn_metric.hip: indices / distances are host arrays, n x k, padded with UINT32_MAX / +inf from column min(k, n - 1) on
void nearest_neighbors_device(const double *d_data, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, uint32_t *indices,
                              double *distances);
// a query set of its own: n_q x k; include_self == false drops the point whose index equals the query's row number
void nearest_neighbors_query_device(const double *d_queries, uint64_t n_q, uint32_t ld_q, const double *d_points, uint64_t n_p, uint32_t ld_p,
                                    uint32_t d, uint32_t k, int kind, bool include_self, uint32_t *indices, double *distances);
// COLLECTIVE, over a sharded point set: d_pts are the rank's own rows [begin, begin + n_local) of the n global ones; indices /
// distances are host arrays over the rank's rows and hold GLOBAL indices. Counts st.knn_blocks / knn_allreduces / knn_blocks_filtered.
struct Storage;
void nearest_neighbors_sharded(Storage &st, const double *d_pts, uint32_t ld, uint64_t begin, uint64_t n_local, uint64_t n, uint32_t d,
                               uint32_t k, int kind, uint32_t *indices, double *distances);
// knn_metric_host.cpp
void host_nearest_neighbors_query(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k, int kind,
                                  bool include_self, uint32_t *indices, double *distances);
void host_nearest_neighbors(const double *data, uint64_t n, uint32_t d, uint32_t k, int kind, uint32_t *indices, double *distances);
void host_distance(int kind, const double *x, const double *y, uint32_t d, double *key, double *dist);
void host_metric_rows(int kind, const double *data, uint64_t n, uint32_t d, double *c, double *s, double *z);
void nearest_neighbors_check_args(uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, bool k_limit = true);

} // namespace scanrs
