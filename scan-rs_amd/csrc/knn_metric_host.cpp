// knn_metric_host.cpp — the host twin of knn_metric.hip: nearest_neighbors (umap-rs/src/knn.rs:112-166) by exhaustive search with the
// reference's own formulas (umap-rs/src/dist.rs:69-124, restated once in knn_metric.hpp), and the helpers the tests of the filtered
// route read. No device. Compiled with -ffp-contract=off like the kernels: the answers are equal bit for bit.
#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>

#include "common.hpp"
#include "host_team.hpp"
#include "knn_metric.hpp"

namespace scanrs {

using namespace knn_metric;

// k_limit: the device search keeps its k-lists in a thread's private memory (k <= 128); the host twin takes any k
void nearest_neighbors_check_args(uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, bool k_limit) {
    if (kind != EUCLIDEAN && kind != PEARSON && kind != COSINE)
        fail(SCANRS_ERR_ARGUMENT, "nearest_neighbors: distance type %d (0 euclidean, 1 pearson, 2 cosine)", kind);
    if (k_limit && k > 128) fail(SCANRS_ERR_ARGUMENT, "nearest_neighbors: k must not exceed 128");
    if (d == 0 || d > 128) fail(SCANRS_ERR_ARGUMENT, "nearest_neighbors: 1 <= dimensions <= 128");
    if (ld < d) fail(SCANRS_ERR_ARGUMENT, "nearest_neighbors: leading dimension smaller than the number of coordinates");
    if (n > 0xFFFFFFFEull) fail(SCANRS_ERR_SHAPE, "nearest_neighbors: too many points for u32 indices");
}

namespace {

// the squared distance as scanrs_knn forms it (knn.hip): one fma chain over the squared differences, in coordinate order
inline double sq_dist(const double *q, const double *p, uint32_t d) {
    double s = 0.0;
    for (uint32_t j = 0; j < d; j++) {
        const double t = p[j] - q[j];
        s = std::fma(t, t, s);
    }
    return s;
}
inline double dot(const double *x, const double *y, uint32_t d) {
    double s = 0.0;
    for (uint32_t j = 0; j < d; j++) s = s + x[j] * y[j];
    return s;
}
void refuse_not_finite(const double *data, uint64_t n, uint32_t d, const char *what) {
    for (uint64_t r = 0; r < n; r++)
        for (uint32_t j = 0; j < d; j++)
            if (!std::isfinite(data[r * d + j]))
                fail(SCANRS_ERR_ARGUMENT, "nearest_neighbors: row %llu of the %s holds a coordinate that is not finite", (unsigned long long)r, what);
}

} // namespace

void host_distance(int kind, const double *x, const double *y, uint32_t d, double *key, double *dist) {
    if (kind == EUCLIDEAN) {
        *key = *dist = std::sqrt(sq_dist(x, y, d));
        return;
    }
    std::vector<double> cx(d), cy(d);
    const double s_xx = prepare_row(kind, x, d, cx.data(), nullptr), s_yy = prepare_row(kind, y, d, cy.data(), nullptr);
    const double kq = std::sqrt(pair_value(s_xx, s_yy, dot(cx.data(), cy.data(), d)));
    *key = kq;
    *dist = kq * kq; // metric2dist (dist.rs:24, 32): generally not the bits of D
}

void host_metric_rows(int kind, const double *data, uint64_t n, uint32_t d, double *c, double *s, double *z) {
    for (uint64_t r = 0; r < n; r++) s[r] = prepare_row(kind, data + r * d, d, c + r * d, z ? z + r * d : nullptr);
}

namespace {

// every query row against every point row, the point whose index is the query's row number left out when `skip`; both finite
void host_search(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k, int kind, bool skip,
                 uint32_t *indices, double *distances) {
    std::vector<double> cq, sq, cp, sp;
    const double *qrows = queries, *prows = points;
    const bool same = queries == points && n_q == n_p;
    if (kind != EUCLIDEAN) {
        cp.resize(n_p * d);
        sp.resize(n_p);
        host_metric_rows(kind, points, n_p, d, cp.data(), sp.data(), nullptr);
        prows = cp.data();
        if (!same) {
            cq.resize(n_q * d);
            sq.resize(n_q);
            host_metric_rows(kind, queries, n_q, d, cq.data(), sq.data(), nullptr);
        }
        qrows = same ? cp.data() : cq.data();
    }
    const double *s_q = same ? sp.data() : sq.data(), *s_p = sp.data();
    auto search = [&](uint64_t q) {
        uint32_t *bi = indices + q * k;
        double *bd = distances + q * k; // the rank key while the list is built (squared distance, or sqrt(D))
        uint32_t have = 0;
        for (uint64_t p = 0; p < n_p; p++) {
            if (skip && p == q) continue; // query.idx != idx, knn.rs:155
            const double key = kind == EUCLIDEAN ? sq_dist(qrows + q * d, prows + p * d, d)
                                                 : std::sqrt(pair_value(s_q[q], s_p[p], dot(qrows + q * d, prows + p * d, d)));
            if (have == k && !(key < bd[k - 1])) continue;
            // sorted insertion; equal keys stay in index order because candidates arrive in index order
            uint32_t pos = have < k ? have : k - 1u;
            while (pos > 0 && bd[pos - 1] > key) {
                bd[pos] = bd[pos - 1];
                bi[pos] = bi[pos - 1];
                pos--;
            }
            bd[pos] = key;
            bi[pos] = (uint32_t)p;
            if (have < k) have++;
        }
        for (uint32_t i = 0; i < have; i++) bd[i] = kind == EUCLIDEAN ? std::sqrt(bd[i]) : bd[i] * bd[i];
        for (uint32_t i = have; i < k; i++) { // the reference's initial fill, knn.rs:139-140
            bi[i] = 0xFFFFFFFFu;
            bd[i] = INFINITY;
        }
    };
    int T = (int)std::min<uint64_t>({8, std::max(1u, std::thread::hardware_concurrency()), n_q * n_p * d / (1u << 22) + 1});
    HostTeam *team = T > 1 ? HostTeam::acquire(T) : nullptr;
    if (!team) T = 1;
    auto part = [&](int t) {
        for (uint64_t q = (uint64_t)t; q < n_q; q += (uint64_t)T) search(q);
    };
    if (team) team->start(T, part);
    part(0);
    if (team) {
        team->join();
        team->release();
    }
}

} // namespace

void host_nearest_neighbors(const double *data, uint64_t n, uint32_t d, uint32_t k, int kind, uint32_t *indices, double *distances) {
    nearest_neighbors_check_args(n, d, d, k, kind, false);
    if (k == 0 || n == 0) return;
    refuse_not_finite(data, n, d, "data");
    host_search(data, n, data, n, d, k, kind, true, indices, distances);
}

void host_nearest_neighbors_query(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k, int kind,
                                  bool include_self, uint32_t *indices, double *distances) {
    nearest_neighbors_check_args(n_p, d, d, k, kind, false);
    nearest_neighbors_check_args(n_q, d, d, k, kind, false);
    if (k == 0 || n_q == 0) return;
    refuse_not_finite(queries, n_q, d, "queries");
    refuse_not_finite(points, n_p, d, "points");
    host_search(queries, n_q, points, n_p, d, k, kind, !include_self, indices, distances);
}


} // namespace scanrs
