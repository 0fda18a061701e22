// fuzzy_host.cpp — fuzzy_simplicial_set without a device (the twin of fuzzy.hip: the same arithmetic through fuzzy.hpp, so the
// device equals it in every bit), the host-only pieces the tests pin the reference's tables with, and the C entry points of the
// scanrs_graph block of scanrs_amd.h. DESIGN.md §7r. Built with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <memory>

#include "fuzzy_graph.hpp"
#include "knn_metric.hpp"

namespace scanrs {

using namespace fuzzy;

FuzzyParams fuzzy_resolve(const char *name, const scanrs_fuzzy_params *p, uint64_t n, uint32_t k) {
    if (!p) fail(SCANRS_ERR_ARGUMENT, "null argument");
    if (n == 0 || k == 0) fail(SCANRS_ERR_ARGUMENT, "%s: no rows or no columns in the neighbour lists (the reference asserts)", name);
    if (k > FZ_KMAX) fail(SCANRS_ERR_ARGUMENT, "%s: k must not exceed %u", name, FZ_KMAX);
    if (n > 0xFFFFFFFEull) fail(SCANRS_ERR_ARGUMENT, "%s: at most 2^32 - 2 rows", name);
    if (!std::isfinite(p->local_connectivity) || p->local_connectivity < 0.0)
        fail(SCANRS_ERR_ARGUMENT, "%s: local_connectivity must be finite and not negative", name);
    if (!std::isfinite(p->set_op_mix_ratio)) fail(SCANRS_ERR_ARGUMENT, "%s: set_op_mix_ratio must be finite", name);
    if (std::isnan(p->bandwidth)) fail(SCANRS_ERR_ARGUMENT, "%s: bandwidth is NaN", name);
    FuzzyParams P;
    P.local_connectivity = p->local_connectivity;
    P.set_op_mix_ratio = p->set_op_mix_ratio;
    P.combine = p->apply_fuzzy_combine != 0;
    P.n_iter = p->n_iter ? p->n_iter : FZ_NITER;
    P.bandwidth = p->bandwidth == 0.0 ? FZ_BANDWIDTH : p->bandwidth;
    P.target = std::log2((double)k) * P.bandwidth;
    return P;
}

void fuzzy_refuse_row(const char *name, unsigned long long code) {
    if (code == ~0ull) return;
    const unsigned long long row = code >> 2;
    switch ((int)(code & 3)) {
    case FZ_BAD_NAN: fail(SCANRS_ERR_ARGUMENT, "%s: row %llu of the distances holds a NaN", name, row);
    case FZ_BAD_INDEX: fail(SCANRS_ERR_ARGUMENT, "%s: row %llu of the indices names a row that does not exist (and is not UINT32_MAX)", name, row);
    case FZ_BAD_RHO:
        fail(SCANRS_ERR_ARGUMENT, "%s: row %llu has too few non-zero distances for this local_connectivity (the reference indexes past their end)",
             name, row);
    default: fail(SCANRS_ERR_ARGUMENT, "%s: row %llu of the indices names a row twice", name, row);
    }
}

namespace {

struct HostRow {
    const double *p;
    double operator()(uint32_t j) const { return p[j]; }
};

// the edge list of a CSR graph in host memory (embedding.rs:38-53, 75-85, without the shuffle)
uint64_t host_edges(const scanrs_graph &g, double n_epochs, uint32_t *head, uint32_t *tail, double *weights, double *eps) {
    double graph_max = 0.0;
    for (uint64_t e = 0; e < g.nnz; e++) graph_max = fz_max(graph_max, g.values[e]);
    const double threshold = graph_max / n_epochs;
    double max_w = -DBL_MAX;
    uint64_t count = 0;
    for (uint64_t r = 0; r < g.n; r++)
        for (uint64_t e = g.indptr[r]; e < g.indptr[r + 1]; e++) {
            const double v = g.values[e];
            if (!fz_edge_kept(v, threshold)) continue;
            if (weights) tail[count] = (uint32_t)r, head[count] = g.indices[e], weights[count] = v;
            max_w = fz_max(max_w, v);
            count++;
        }
    if (weights)
        for (uint64_t e = 0; e < count; e++) eps[e] = fz_epochs_per_sample(weights[e], max_w, n_epochs);
    return count;
}

void host_fuzzy(const char *name, const uint32_t *idx, const double *dist, uint64_t n, uint32_t k, const FuzzyParams &P, scanrs_graph &g) {
    // the refusals: the first row, and within it the smallest kind
    std::vector<double> rho(n, 0.0);
    unsigned long long bad = ~0ull;
    for (uint64_t i = 0; i < n && bad == ~0ull; i++) {
        const uint32_t *ri = idx + i * k;
        const double *rd = dist + i * k;
        int kind = 4;
        for (uint32_t j = 0; j < k; j++) {
            if (rd[j] != rd[j]) kind = std::min<int>(kind, FZ_BAD_NAN);
            if (ri[j] != FZ_NO_INDEX && ri[j] >= n) kind = std::min<int>(kind, FZ_BAD_INDEX);
            if (ri[j] != FZ_NO_INDEX)
                for (uint32_t j2 = 0; j2 < j; j2++)
                    if (ri[j2] == ri[j]) kind = std::min<int>(kind, FZ_BAD_REPEAT);
        }
        if (!fz_rho(HostRow{rd}, k, P.local_connectivity, &rho[i])) kind = std::min<int>(kind, FZ_BAD_RHO);
        if (kind < 4) bad = i * 4ull + (unsigned long long)kind;
    }
    fuzzy_refuse_row(name, bad);
    std::vector<double> sigma(n), fold(n);
    for (uint64_t i = 0; i < n; i++) {
        const HostRow row{dist + i * k};
        sigma[i] = fz_smooth_knn_dist(row, k, rho[i], P.target, P.n_iter, nullptr);
        fold[i] = fz_row_fold(row, k);
        if (rho[i] > 0.0) sigma[i] = fz_floor_row(sigma[i], fold[i], k);
    }
    // Stated deviation: the reference's global mean is one sequential fold over all n * k distances; here the row folds
    // are added in a fixed tree. It reaches only sigma of rows whose rho is not > 0.
    const double total = fz_tree_host(fold.data(), n);
    for (uint64_t i = 0; i < n; i++)
        if (!(rho[i] > 0.0)) sigma[i] = fz_floor_global(sigma[i], total, n, k);
    // R[index, i] (fuzzy.rs:173-175: row = the neighbour, column = i), then its transpose; sorted by (row, column), stable
    struct Entry {
        uint64_t key;
        double v;
    };
    std::vector<Entry> ent;
    ent.reserve((P.combine ? 2 : 1) * n * k);
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t j = 0; j < k; j++) {
            const uint32_t c = idx[i * k + j];
            if (c == FZ_NO_INDEX) continue;
            ent.push_back({((uint64_t)c << 32) | i, fz_membership(j, c, dist[i * k + j], rho[i], sigma[i])});
        }
    if (P.combine) {
        const size_t m = ent.size();
        for (size_t e = 0; e < m; e++) ent.push_back({(ent[e].key << 32) | (ent[e].key >> 32), ent[e].v});
    }
    std::stable_sort(ent.begin(), ent.end(), [](const Entry &a, const Entry &b) { return a.key < b.key; });
    g.n = n, g.k = k, g.on_device = false;
    g.indptr.assign(n + 1, 0);
    g.indices.clear(), g.values.clear();
    for (size_t e = 0; e < ent.size();) {
        const bool two = e + 1 < ent.size() && ent[e + 1].key == ent[e].key;
        g.indices.push_back((uint32_t)(ent[e].key & 0xFFFFFFFFu));
        g.values.push_back(P.combine ? fz_union(ent[e].v, two ? ent[e + 1].v : 0.0, P.set_op_mix_ratio) : ent[e].v);
        g.indptr[(ent[e].key >> 32) + 1]++;
        e += two ? 2 : 1;
    }
    for (uint64_t r = 0; r < n; r++) g.indptr[r + 1] += g.indptr[r];
    g.nnz = g.values.size();
    g.sigmas = std::move(sigma);
    g.rhos = std::move(rho);
}

void need_graph(const scanrs_graph *g) {
    if (!g) fail(SCANRS_ERR_ARGUMENT, "null handle");
}
void need_epochs(double n_epochs) {
    if (!(n_epochs > 0.0)) fail(SCANRS_ERR_ARGUMENT, "graph_edges: n_epochs must be > 0");
}

// the lists from host arrays into device memory, then the device chain
void fuzzy_from_host(const uint32_t *idx, const double *dist, uint64_t n, uint32_t k, const scanrs_fuzzy_params *params, scanrs_graph **out) {
    const char *name = "fuzzy_simplicial_set";
    if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
    *out = nullptr;
    const FuzzyParams P = fuzzy_resolve(name, params, n, k);
    if (!idx || !dist) fail(SCANRS_ERR_ARGUMENT, "null argument");
    need_device();
    std::unique_ptr<scanrs_graph> g(new scanrs_graph());
    {
        DevBuf<uint32_t> di(n * k);
        DevBuf<double> dd(n * k);
        SCANRS_HIP(hipMemcpy(di.p, idx, n * k * 4, hipMemcpyHostToDevice));
        SCANRS_HIP(hipMemcpy(dd.p, dist, n * k * 8, hipMemcpyHostToDevice));
        fuzzy_device(name, di.p, dd.p, n, k, k, P, *g);
    }
    device_free_flush();
    *out = g.release();
}

void umap_graph_on_device(const double *d_points, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, const FuzzyParams &P, uint32_t k_eff,
                          scanrs_graph &g) {
    DevBuf<uint32_t> idx;
    DevBuf<double> dist;
    nearest_neighbors_resident(d_points, n, ld, d, k_eff, kind, idx, dist);
    fuzzy_device("umap_graph", idx.p, dist.p, n, k_eff, k_eff, P, g);
}

// the checks of scanrs_nearest_neighbors, then those of the graph on the width the reference would return (knn.rs:124-127)
uint32_t umap_graph_width(const scanrs_fuzzy_params *params, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, FuzzyParams &P) {
    nearest_neighbors_check_args(n, ld, d, k, kind);
    const uint32_t k_eff = (uint32_t)std::min<uint64_t>(k, n ? n - 1 : 0);
    P = fuzzy_resolve("umap_graph", params, n, k_eff);
    return k_eff;
}

} // namespace
} // namespace scanrs

using namespace scanrs;

extern "C" {

int scanrs_fuzzy_simplicial_set(const uint32_t *knn_indices, const double *knn_distances, uint64_t n, uint32_t k, const scanrs_fuzzy_params *params,
                                scanrs_graph **out) {
    const int rc = guard([&] { fuzzy_from_host(knn_indices, knn_distances, n, k, params, out); });
    if (rc != SCANRS_OK) device_free_flush();
    return rc;
}
int scanrs_fuzzy_simplicial_set_device(const uint32_t *d_knn_indices, const double *d_knn_distances, uint64_t n, uint32_t ld, uint32_t k,
                                       const scanrs_fuzzy_params *params, scanrs_graph **out) {
    const int rc = guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = nullptr;
        const FuzzyParams P = fuzzy_resolve("fuzzy_simplicial_set", params, n, k);
        if (!d_knn_indices || !d_knn_distances) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (ld < k) fail(SCANRS_ERR_ARGUMENT, "fuzzy_simplicial_set: leading dimension smaller than the width of the lists");
        need_device();
        std::unique_ptr<scanrs_graph> g(new scanrs_graph());
        fuzzy_device("fuzzy_simplicial_set", d_knn_indices, d_knn_distances, n, ld, k, P, *g);
        *out = g.release();
    });
    device_free_flush();
    return rc;
}
int scanrs_umap_graph(const double *points, uint64_t n, uint32_t d, uint32_t k, int distance_type, const scanrs_fuzzy_params *params,
                      scanrs_graph **out) {
    const int rc = guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = nullptr;
        FuzzyParams P;
        const uint32_t k_eff = umap_graph_width(params, n, d, d, k, distance_type, P);
        if (!points) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_device();
        std::unique_ptr<scanrs_graph> g(new scanrs_graph());
        {
            DevBuf<double> dp(n * d);
            SCANRS_HIP(hipMemcpy(dp.p, points, n * d * 8, hipMemcpyHostToDevice));
            umap_graph_on_device(dp.p, n, d, d, k, distance_type, P, k_eff, *g);
        }
        *out = g.release();
    });
    device_free_flush();
    return rc;
}
int scanrs_umap_graph_device(const double *d_points, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int distance_type,
                             const scanrs_fuzzy_params *params, scanrs_graph **out) {
    const int rc = guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = nullptr;
        FuzzyParams P;
        const uint32_t k_eff = umap_graph_width(params, n, ld, d, k, distance_type, P);
        if (!d_points) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_device();
        std::unique_ptr<scanrs_graph> g(new scanrs_graph());
        umap_graph_on_device(d_points, n, ld, d, k, distance_type, P, k_eff, *g);
        *out = g.release();
    });
    device_free_flush();
    return rc;
}
int scanrs_host_fuzzy_simplicial_set(const uint32_t *knn_indices, const double *knn_distances, uint64_t n, uint32_t k,
                                     const scanrs_fuzzy_params *params, scanrs_graph **out) {
    return guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = nullptr;
        const FuzzyParams P = fuzzy_resolve("fuzzy_simplicial_set", params, n, k);
        if (!knn_indices || !knn_distances) fail(SCANRS_ERR_ARGUMENT, "null argument");
        std::unique_ptr<scanrs_graph> g(new scanrs_graph());
        host_fuzzy("fuzzy_simplicial_set", knn_indices, knn_distances, n, k, P, *g);
        *out = g.release();
    });
}
void scanrs_graph_free(scanrs_graph *g) {
    if (!g) return;
    const bool dev = g->on_device;
    delete g;
    if (dev) device_free_flush();
}
int scanrs_graph_info(const scanrs_graph *g, uint64_t *out, uint32_t n_out) {
    return guard([&] {
        need_graph(g);
        if (!out && n_out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        const uint64_t v[4] = {g->n, g->nnz, g->k, g->on_device ? 1ull : 0ull};
        for (uint32_t i = 0; i < n_out; i++) out[i] = i < 4 ? v[i] : 0;
    });
}
int scanrs_graph_to_host(const scanrs_graph *g, uint64_t *indptr, uint32_t *indices, double *values) {
    return guard([&] {
        need_graph(g);
        if (!indptr || ((!indices || !values) && g->nnz)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (g->on_device) {
            SCANRS_D2H(indptr, g->d_indptr.p, (g->n + 1) * 8, 0);
            if (g->nnz) {
                SCANRS_D2H(indices, g->d_indices.p, g->nnz * 4, 0);
                SCANRS_D2H(values, g->d_values.p, g->nnz * 8, 0);
            }
        } else {
            std::copy(g->indptr.begin(), g->indptr.end(), indptr);
            std::copy(g->indices.begin(), g->indices.end(), indices);
            std::copy(g->values.begin(), g->values.end(), values);
        }
    });
}
int scanrs_graph_sigmas_rhos(const scanrs_graph *g, double *sigmas, double *rhos) {
    return guard([&] {
        need_graph(g);
        if (!sigmas || !rhos) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (g->on_device) {
            SCANRS_D2H(sigmas, g->d_sigmas.p, g->n * 8, 0);
            SCANRS_D2H(rhos, g->d_rhos.p, g->n * 8, 0);
        } else {
            std::copy(g->sigmas.begin(), g->sigmas.end(), sigmas);
            std::copy(g->rhos.begin(), g->rhos.end(), rhos);
        }
    });
}
int scanrs_graph_device(const scanrs_graph *g, const uint64_t **d_indptr, const uint32_t **d_indices, const double **d_values) {
    return guard([&] {
        need_graph(g);
        if (!g->on_device) fail(SCANRS_ERR_ARGUMENT, "graph_device: this graph lives in host memory (scanrs_host_fuzzy_simplicial_set)");
        if (d_indptr) *d_indptr = reinterpret_cast<const uint64_t *>(g->d_indptr.p);
        if (d_indices) *d_indices = g->d_indices.p;
        if (d_values) *d_values = g->d_values.p;
    });
}
int scanrs_graph_edge_count(const scanrs_graph *g, double n_epochs, uint64_t *count) {
    const int rc = guard([&] {
        need_graph(g);
        if (!count) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_epochs(n_epochs);
        if (g->on_device)
            fuzzy_edges_device(*g, n_epochs, count, nullptr, nullptr, nullptr, nullptr);
        else
            *count = host_edges(*g, n_epochs, nullptr, nullptr, nullptr, nullptr);
    });
    if (g && g->on_device) device_free_flush();
    return rc;
}
int scanrs_graph_edges(const scanrs_graph *g, double n_epochs, uint32_t *head, uint32_t *tail, double *weights, double *epochs_per_sample) {
    const int rc = guard([&] {
        need_graph(g);
        need_epochs(n_epochs);
        uint64_t count = 0;
        if (g->on_device) {
            fuzzy_edges_device(*g, n_epochs, &count, nullptr, nullptr, nullptr, nullptr);
            if (count && (!head || !tail || !weights || !epochs_per_sample)) fail(SCANRS_ERR_ARGUMENT, "null argument");
            if (count) fuzzy_edges_device(*g, n_epochs, &count, head, tail, weights, epochs_per_sample);
        } else {
            count = host_edges(*g, n_epochs, nullptr, nullptr, nullptr, nullptr);
            if (count && (!head || !tail || !weights || !epochs_per_sample)) fail(SCANRS_ERR_ARGUMENT, "null argument");
            if (count) host_edges(*g, n_epochs, head, tail, weights, epochs_per_sample);
        }
    });
    if (g && g->on_device) device_free_flush();
    return rc;
}
int scanrs_host_fuzzy_exp(const double *x, uint64_t count, double *out) {
    return guard([&] {
        if (count && (!x || !out)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        for (uint64_t i = 0; i < count; i++) out[i] = fz_exp(x[i]);
    });
}
int scanrs_host_smooth_knn_dist(const double *distances, uint32_t k, double rho, double bandwidth, uint32_t n_iter, double *sigma,
                                uint32_t *iterations) {
    return guard([&] {
        if (!distances || !sigma) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (k == 0) fail(SCANRS_ERR_ARGUMENT, "smooth_knn_dist: no distances");
        const double target = std::log2((double)k) * (bandwidth == 0.0 ? FZ_BANDWIDTH : bandwidth);
        uint32_t it = 0;
        *sigma = fz_smooth_knn_dist(HostRow{distances}, k, rho, target, n_iter ? n_iter : FZ_NITER, &it);
        if (iterations) *iterations = it;
    });
}
int scanrs_host_membership_strengths(const uint32_t *knn_indices, const double *knn_distances, uint64_t n, uint32_t k, const double *sigmas,
                                     const double *rhos, uint32_t *rows, uint32_t *cols, double *values, uint64_t *count) {
    return guard([&] {
        if (!count || ((!knn_indices || !knn_distances || !sigmas || !rhos || !rows || !cols || !values) && n && k))
            fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (n == 0 || k == 0) fail(SCANRS_ERR_ARGUMENT, "membership_strengths: empty neighbour lists (the reference asserts)");
        uint64_t m = 0;
        for (uint64_t i = 0; i < n; i++)
            for (uint32_t j = 0; j < k; j++) {
                const uint32_t c = knn_indices[i * k + j];
                if (c == FZ_NO_INDEX) continue;
                cols[m] = (uint32_t)i, rows[m] = c;
                values[m] = fz_membership(j, c, knn_distances[i * k + j], rhos[i], sigmas[i]);
                m++;
            }
        *count = m;
    });
}

} // extern "C"
