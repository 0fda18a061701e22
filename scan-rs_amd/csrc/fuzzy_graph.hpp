// fuzzy_graph.hpp — the handle behind scanrs_graph and what fuzzy_host.cpp (the twin, the C entry points) and fuzzy.hip (the device
// chain) call of each other. DESIGN.md §7r.
#pragma once
#include <vector>

#include "common.hpp"
#include "fuzzy.hpp"

// The UMAP graph in CSR: either resident on the device (the device entry points) or in host memory (the twin). Both answer the
// same accessors; scanrs_graph_device refuses a host graph.
struct scanrs_graph {
    uint64_t n = 0, nnz = 0;
    uint32_t k = 0; // the width of the lists it was made from
    bool on_device = false;
    scanrs::DevBuf<unsigned long long> d_indptr; // n + 1
    scanrs::DevBuf<uint32_t> d_indices;          // nnz, ascending within a row
    scanrs::DevBuf<double> d_values, d_sigmas, d_rhos;
    std::vector<uint64_t> indptr;
    std::vector<uint32_t> indices;
    std::vector<double> values, sigmas, rhos;
};

namespace scanrs {

struct FuzzyParams { // scanrs_fuzzy_params with the defaults filled in
    double local_connectivity, set_op_mix_ratio;
    bool combine;
    uint32_t n_iter;
    double bandwidth;
    double target; // log2(k) * bandwidth (fuzzy.rs:118), formed once on the host for the twin and the device alike
};
// the refusals that need no look at the lists; `name`: the entry point in their texts
FuzzyParams fuzzy_resolve(const char *name, const scanrs_fuzzy_params *p, uint64_t n, uint32_t k);
void fuzzy_refuse_row(const char *name, unsigned long long code); // code = row * 4 + kind (fuzzy.hpp); ~0: nothing to refuse
// fuzzy.hip. The lists are in device memory, n x k with leading dimension ld.
void fuzzy_device(const char *name, const uint32_t *d_idx, const double *d_dist, uint64_t n, uint32_t ld, uint32_t k, const FuzzyParams &P,
                  scanrs_graph &g);
// count only where weights is null
void fuzzy_edges_device(const scanrs_graph &g, double n_epochs, uint64_t *count, uint32_t *head, uint32_t *tail, double *weights,
                        double *epochs_per_sample);
// knn_metric.hip: the search of nearest_neighbors with its lists left in device memory, n x k (k <= n - 1: no padding)
void nearest_neighbors_resident(const double *d_data, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, DevBuf<uint32_t> &idx,
                                DevBuf<double> &dist);

} // namespace scanrs
